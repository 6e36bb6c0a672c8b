"""Lowering of the reference's nn.Module graphs onto libv2v_hip.so.

The reference describes every network as nn.Sequential lists of Conv2d / ConvTranspose2d /
ReflectionPad2d / BatchNorm2d / InstanceNorm2d / ReLU / LeakyReLU / Tanh / Sigmoid /
ResnetBlock (models/networks.py:117-725).  `Engine.run_sequential` walks such a list and
emits the fused HIP launches:

    [ReflectionPad2d(p)] Conv2d|ConvTranspose2d  ->  v2v_conv2d (padding folded into the loader)
       + norm [+ act]                            ->  conv(raw + statistics), v2v_bn_finalize,
                                                     v2v_bn_apply (normalise + act + residual adds)
       + act only / nothing                      ->  activation in the conv epilogue
    ResnetBlock                                   ->  two of the above, residual in bn_apply

All tensors handed to the library are NHWC with a channel stride padded to 16 bytes.  The
emitted launches either run immediately (eager) or are recorded into a `Plan` that is then
replayed per frame as one native call (hipGraphs, one per lane segment).  No torch compute op is on this path.
"""
import contextlib
import ctypes as C
import json
import math
import os
import sys

import torch
import torch.nn as nn

from . import lib as L
from .lib import lib, check, ConvDesc
# Which tile a launch may try -- the tile-table views, the eligibility predicates, the candidate lists -- is tile_search.py's; the
# names that tests, scripts and bench.py read from this module stay importable from it.
from . import tile_search as TS
from .tile_search import (TILE_CFGS, PATCH_CFGS, S2_CFGS, T2_CFGS, S7_CFGS, ABLATION_TILES, PAIR_TILES, BWD_PATCH_TILES,      # noqa: F401
                          ONE_TILES, PERSISTENT_TILES, ONE_FIN, EXP_TILES, HEAD_TILE, C8_TILE, ROWSUM_TILE, tile_korder,
                          is_patch_tile, _flag, _cfg3)

_TORCH_DTYPE = {L.F32: torch.float32, L.BF16: torch.bfloat16}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_HAS_GPU = []


def _stream():
    """hipStream_t of torch's current stream.  (torch.cuda.is_available() re-reads the environment on every call: 4400 calls =
    ~8 ms of a 75 ms host-bound training chunk, scripts/host_profile_train.py -- its answer cannot change, so it is asked once.)"""
    if not _HAS_GPU:
        _HAS_GPU.append(torch.cuda.is_available())
    if not _HAS_GPU[0]:
        return None          # record-only dry runs on a CPU host never launch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def vec_of(dtype):
    return 8 if dtype == L.BF16 else 4


def pad_channels(c, dtype):
    v = vec_of(dtype)
    return (c + v - 1) // v * v


class Act:
    """NHWC activation: tensor [N,H,W,Cs] (Cs = padded channel stride), C real channels."""
    __slots__ = ("t", "C", "onehot", "x3")

    def __init__(self, t, C, onehot=None):
        self.t, self.C = t, C
        self.onehot = onehot      # LabelSource when this Act is the one-hot encoding of label maps (encode_labels)
        self.x3 = None            # x3 engines: the same values as a bf16x3 operand [hi | lo | hi], written by the producing bn_apply

    def detach(self):
        return Act(self.t.detach(), self.C)

    @property
    def N(self): return self.t.shape[0]
    @property
    def H(self): return self.t.shape[1]
    @property
    def W(self): return self.t.shape[2]
    @property
    def Cs(self): return self.t.stride(2)      # true channel stride (a channel-sliced view keeps its parent's)


class LabelSource:
    """The label / instance maps an encoded one-hot Act was built from: [T][H][W] fp32-encoded integers or uint8 / int32.
    A 7x7 stem convolution over such an Act runs as a weight gather-sum on the maps (csrc/onehot_stem.hip)."""
    __slots__ = ("labels", "inst", "T", "label_nc", "codes")

    def __init__(self, labels, inst, T, label_nc):
        self.labels, self.inst, self.T, self.label_nc = labels, inst, T, label_nc
        self.codes = None         # [T][H][W] uint8 label | edge << 7 (Engine.label_codes): what the stem kernels stage from


_PARAM_EPOCH = [0]


def bump_param_epoch():
    """Force every packed weight copy to be refreshed on next use (parameters changed behind torch's back by
    something other than optim.FusedAdam, which bumps the per-buffer counter of its own parameters instead -- frozen
    networks such as FlowNet2 / VGG19 are then never re-packed by a training step)."""
    _PARAM_EPOCH[0] += 1


_ENGINES = []        # weak references to every live Engine (repack_after_step walks them)


def repack_after_step(flat=None):
    """optim.FusedAdam.step, after its update kernel: re-pack -- on each engine's side stream -- every packed weight copy that
    was in use and is now stale.  Lazily, the training step re-packed each layer in front of its first use of the next chunk:
    ~270 small launches per 512x256 chunk in the serial chain of the forward / backward passes (5 % of the step's kernel time
    plus their launch turnarounds, profiles/r06_v1_train_kernel_stats.txt).  Issued here they run beside the next backward
    pass; the compute stream waits for them once, at the engine's next convolution (Engine.wait_repack)."""
    for ref in list(_ENGINES):
        eng = ref()
        if eng is None:
            _ENGINES.remove(ref)
        else:
            eng.repack_async(flat)


class PackedConv:
    """Device-resident packed weights of one nn.Conv2d / nn.ConvTranspose2d.

    role 'fwd':   the layer's own operator.
    role 'bwd':   its backward-data operator -- the SAME parameter tensor read with the roles of
                  cin / cout swapped (include/v2v_hip.h, v2v_conv2d): a Conv2d becomes a transposed conv
                  (stride s; pad p, or pad 0 behind a ReflectionPad2d), a ConvTranspose2d a stride-2 Conv2d.
    """

    def __init__(self, eng, mod, cin_stride, role="fwd", reflect=False, korder=0):
        self.mod = mod
        self.role = role
        self.korder = korder      # 0: tap-major K (implicit-GEMM tiles), 1: channel-chunk-major (patch kernel), 3: paired-x (PairedXConv)
        self.src_mod = None       # korder 3: the geometry below is the layer's own, the packed matrix its PairedXConv's (64 x 9 x 64, chunk-major)
        if korder == 3:
            if role != "fwd" or cin_stride != 32:
                raise ValueError("paired-x packing: forward operator of a layer with 64-byte pixels")
            self.src_mod = PairedXConvT(mod) if isinstance(mod, nn.ConvTranspose2d) else PairedXConv(mod)
        mod_t = getattr(mod, "is_transposed", isinstance(mod, nn.ConvTranspose2d))
        w = mod.weight
        self.KH, self.KW = mod.kernel_size
        self.stride = mod.stride[0]
        if mod_t:
            m_cin, m_cout = w.shape[0], w.shape[1]
            if tuple(mod.stride) != (2, 2):
                raise NotImplementedError("ConvTranspose2d must be stride 2")
        else:
            m_cout, m_cin = w.shape[0], w.shape[1]
        if role == "fwd":
            self.transposed = mod_t
            self.cin, self.cout = m_cin, m_cout
            self.pad = mod.padding[0]
        else:
            self.transposed = not mod_t
            self.cin, self.cout = m_cout, m_cin          # dY channels in, dX channels out
            self.pad = 0 if reflect else mod.padding[0]
        self.out_pad = mod.output_padding[0] if mod_t else 0
        self.cin_stride = cin_stride
        self.dtype = eng.dtype
        if korder == 4 and (role != "bwd" or mod_t or (self.KH, self.KW) != (3, 3) or self.stride != 1):
            raise ValueError("korder 4: the backward-data operator of a 3x3 / stride 1 Conv2d, packed as a convolution with flipped taps")
        if korder == 5 and (role != "bwd" or mod_t or self.KH != self.KW or self.KH % 2 == 0 or self.stride != 1):
            raise ValueError("korder 5: the backward-data operator of a square stride-1 Conv2d, packed tap-major as a convolution with flipped taps")
        n = ((lib.v2v_conv_packed_elems(64, 64, 32, 3, 3, 1, 2, 1, eng.dtype) if mod_t else lib.v2v_conv_packed_elems(64, 64, 64, 3, 3, 0, 1, self.pad, eng.dtype))
             if korder == 3 else
             lib.v2v_conv_packed_elems(self.cin, cin_stride, self.cout, 3, 3, 0, 1, 1, eng.dtype) if korder == 4 else
             lib.v2v_conv_packed_elems(self.cin, cin_stride, self.cout, self.KH, self.KW, 0, 1, self.KH // 2, eng.dtype) if korder == 5 else
             lib.v2v_conv_packed_elems(self.cin, cin_stride, self.cout, self.KH, self.KW,
                                       int(self.transposed), self.stride, self.pad, eng.dtype))
        self.buf = torch.empty(n, dtype=_TORCH_DTYPE[eng.dtype], device=eng.device)
        self.bias = None
        self.version = None
        self.used = True          # fetched since the last asynchronous re-pack (Engine.repack_async only refreshes what is in use)
        # the flat optimizer buffer that owns this layer's parameter (None: not managed by a FusedAdam, or a composed view such as
        # MergedConv whose `weight` is assembled on read): repack_after_step walks only the packings of the buffer that was stepped --
        # an engine shared by several models (bench.py builds a dozen) holds thousands of packings
        w_own = mod.__dict__.get("_parameters", {}).get("weight") if isinstance(mod, nn.Module) else None
        self.flat_id = id(getattr(w_own, "_v2v_flat", None)) if w_own is not None and getattr(w_own, "_v2v_flat", None) is not None else None
        self.refresh()

    def refresh(self, force=False):
        """(Re)pack if the parameter changed (optimizer step / load_state_dict)."""
        if self.src_mod is not None:               # paired-x: the 64 -> 64 matrix of the PairedXConv, as a chunk-major (korder 1) packing
            ver = self.src_mod.version_key()
            if not force and ver == self.version:
                return
            w32 = self.src_mod.weight.contiguous()
            if self.src_mod.is_transposed:           # 64 -> 32 transposed: the full-tap chunk-major matrix (korder 2) tile 114 reads
                check(lib.v2v_conv_pack_weights(_ptr(w32), _ptr(self.buf), 64, 64, 32, 3, 3, 1, 2, 1, self.dtype, 2, _stream()),
                      "conv_pack_weights (paired-x, transposed)")
            else:
                check(lib.v2v_conv_pack_weights(_ptr(w32), _ptr(self.buf), 64, 64, 64, 3, 3, 0, 1, self.pad, self.dtype, 1, _stream()),
                      "conv_pack_weights (paired-x)")
            self.bias = None if self.mod.bias is None else self.mod.bias.detach().float().contiguous()      # the layer's own 32 values (the kernel folds the index)
            self.version = ver
            return
        if hasattr(self.mod, "version_key"):       # MergedConv: `weight` is a fresh torch.cat on every read (version 0, recycled
            ver = self.mod.version_key()           # address) -- the key comes from the two source layers
            if not force and ver == self.version:
                return
            w = self.mod.weight
        else:
            w = self.mod.weight
            ver = _param_version(self.mod)
            if not force and ver == self.version:
                return
        w32 = w.detach()
        src_cl = (w32.dtype == torch.float32 and w32.dim() == 4 and not w32.is_contiguous()
                  and w32.permute(0, 2, 3, 1).is_contiguous())          # optim.FlatBuffers: channels-last master weights
        if self.korder in (4, 5):
            src_cl = False                                               # (the flipped packing reads the standard layout only)
        if not src_cl and (w32.dtype != torch.float32 or not w32.is_contiguous()):
            w32 = w32.float().contiguous()
        check(lib.v2v_conv_pack_weights(_ptr(w32), _ptr(self.buf), self.cin, self.cin_stride, self.cout,
                                        self.KH, self.KW, int(self.transposed), self.stride, self.pad, self.dtype,
                                        self.korder + (256 if src_cl else 0), _stream()),
              "conv_pack_weights")
        if self.role == "fwd":
            self.bias = None if self.mod.bias is None else self.mod.bias.detach().float().contiguous()
        self.version = ver


def _param_version(mod):
    """What changes when a layer's weight / bias changes: torch's version counters (in-place writes, load_state_dict),
    the storage address (re-homing into flat buffers), and the update counter of the fused optimizer that owns the
    parameter (optim.FlatBuffers.epoch: its HIP kernel writes are invisible to torch)."""
    w = mod.weight
    box = getattr(w, "_v2v_epoch", None)
    return (w._version, w.data_ptr(), None if mod.bias is None else mod.bias._version, _PARAM_EPOCH[0],
            0 if box is None else box[0])


class MergedConv:
    """Two Conv2d heads of identical geometry reading the same input (model_final_flow / model_final_w,
    models/networks.py:181-183) presented as ONE layer with the output channels concatenated: what PackedConv / Engine.conv
    need of an nn.Conv2d, with `weight` / `bias` assembled from the two source layers on every read (eager use re-packs;
    a recorded plan packs once, like every other layer)."""

    def __init__(self, a, b):
        if (a.kernel_size, a.stride, a.padding, a.in_channels, a.groups) != (b.kernel_size, b.stride, b.padding, b.in_channels, b.groups):
            raise ValueError("merged heads must have the same geometry")
        self.a, self.b = a, b
        self.kernel_size, self.stride, self.padding, self.groups = a.kernel_size, a.stride, a.padding, a.groups
        self.in_channels, self.out_channels = a.in_channels, a.out_channels + b.out_channels
        self.output_padding = (0, 0)

    def version_key(self):
        return _param_version(self.a) + _param_version(self.b)

    @property
    def weight(self):
        return torch.cat([self.a.weight.detach(), self.b.weight.detach()], 0)

    @property
    def bias(self):
        if self.a.bias is None and self.b.bias is None:
            return None
        z = lambda m: m.bias.detach() if m.bias is not None else torch.zeros(m.out_channels, device=m.weight.device)
        return torch.cat([z(self.a), z(self.b)], 0)


class X3Conv:
    """An nn.Conv2d seen by the bf16 kernels as a convolution over the bf16x3 operand (csrc/pointwise.hip, split_x3): the
    input channels are [hi(x) | lo(x) | hi(x)], the weights [hi(W) | hi(W) | lo(W)] -- the product is x * W to ~2^-17
    relative on the bf16 matrix pipe.  What PackedConv / Engine.conv need of an nn.Conv2d, assembled on read."""

    def __init__(self, conv):
        self.src = conv
        self.is_transposed = isinstance(conv, nn.ConvTranspose2d)      # weight [cin][cout][kh][kw]: the input channels are dim 0
        self.kernel_size, self.stride, self.padding, self.groups = conv.kernel_size, conv.stride, conv.padding, conv.groups
        self.in_channels, self.out_channels = 3 * conv.in_channels, conv.out_channels
        self.output_padding = tuple(conv.output_padding) if self.is_transposed else (0, 0)

    def version_key(self):
        return _param_version(self.src)

    @property
    def weight(self):
        w = self.src.weight.detach().float()
        hi = w.bfloat16().float()
        lo = (w - hi).bfloat16().float()
        return torch.cat([hi, hi, lo], 0 if self.is_transposed else 1).contiguous()

    @property
    def bias(self):
        return None if self.src.bias is None else self.src.bias.detach()


class PairedXConv:
    """A 3x3 / stride 1 nn.Conv2d with <= 32 input and exactly 32 output channels, seen as a 64 -> 64 convolution over PAIRS of
    horizontally adjacent pixels: the NHWC tensor [H][W][32] IS [H][W/2][64] (paired pixel X = pixels 2X, 2X+1), and
        out[y][X][a*32+co] = sum W'[a*32+co][b*32+ci][ky][kX] in[y+ky-1][X+kX-1][b*32+ci],   W'[..][ky][kX] = W[co][ci][ky][2kX+b-a-1]
    (zero where that tap index falls outside 0..2).  That puts the 32-channel ResnetBlocks of the finest foreground tower
    (models/networks.py:554-593 at ngf_s = 32: 64-byte pixels, half an LDS-DMA row) on the persistent single-chunk kernels
    (csrc/conv3x3_one_kernel.h) unchanged; the products that are not structural zeros are the layer's own, in the layer's own K order.
    Horizontal reflection in the paired domain is a CLAMP (pixel -1 = pixel 1 is the b = 1 half of paired pixel 0; the other half
    meets zero weights) -- the kernel's pair_x mode.  What PackedConv needs of an nn.Conv2d, assembled on read (include/v2v_hip.h,
    w_korder 3)."""

    def __init__(self, conv):
        if isinstance(conv, nn.ConvTranspose2d) or tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (1, 1) or conv.out_channels != 32 \
                or conv.in_channels > 32 or conv.groups != 1:
            raise ValueError("paired-x packing: 3x3 / stride 1 Conv2d, <= 32 -> 32 channels")
        self.src = conv
        self.is_transposed = False
        self.kernel_size, self.stride, self.padding, self.groups = conv.kernel_size, conv.stride, conv.padding, conv.groups
        self.in_channels, self.out_channels = 64, 64
        self.output_padding = (0, 0)

    def version_key(self):
        return _param_version(self.src)

    @property
    def weight(self):
        w = self.src.weight.detach().float()                     # [32][cin][3][3]
        cin = w.shape[1]
        wp = torch.zeros(2, 32, 2, 32, 3, 3, dtype=torch.float32, device=w.device)      # [a][co][b][ci][ky][kX]
        for a in range(2):
            for b in range(2):
                for kX in range(3):
                    kx = 2 * kX + b - a - 1
                    if 0 <= kx <= 2:
                        wp[a, :, b, :cin, :, kX] = w[:, :, :, kx]
        return wp.view(64, 64, 3, 3)

    @property
    def bias(self):
        return None if self.src.bias is None else torch.cat([self.src.bias.detach(), self.src.bias.detach()], 0)


class PairedXConvT:
    """The transposed counterpart of PairedXConv: a ConvTranspose2d(3x3, stride 2, padding 1, output_padding 1) with <= 32 input and
    exactly 16 output channels (models/networks.py:254-260 at ngf_s = 16: the finest foreground tower's last up-sampling stage), seen
    as a ConvTranspose2d 64 -> 32 over pairs of horizontally adjacent pixels: input [H][W][32] = [H][W/2][64], output [2H][2W][16] =
    [2H][W][32] (paired output pixel = output pixels 2x', 2x'+1; channel e*16+co), with
        W3[b*32+ci][e*16+co][ky][kx'] = W[ci][co][ky][kx],   kx = e+1-2b (kx' = 1),  3+e-2b (kx' = 2),  e-1-2b (kx' = 0)
    (zero where kx falls outside 0..2) -- the persistent transposed tile 114 unchanged."""

    def __init__(self, conv):
        if not isinstance(conv, nn.ConvTranspose2d) or tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (2, 2) \
                or tuple(conv.padding) != (1, 1) or tuple(conv.output_padding) != (1, 1) or conv.out_channels != 16 or conv.in_channels > 32 or conv.groups != 1:
            raise ValueError("paired-x packing: ConvTranspose2d(3x3, s2, p1, op1), <= 32 -> 16 channels")
        self.src = conv
        self.is_transposed = True
        self.kernel_size, self.stride, self.padding, self.groups = conv.kernel_size, conv.stride, conv.padding, conv.groups
        self.in_channels, self.out_channels = 64, 32
        self.output_padding = (1, 1)

    def version_key(self):
        return _param_version(self.src)

    @property
    def weight(self):
        w = self.src.weight.detach().float()                     # [cin][16][3][3]
        cin = w.shape[0]
        w3 = torch.zeros(2, 32, 2, 16, 3, 3, dtype=torch.float32, device=w.device)      # [b][ci][e][co][ky][kx']
        for b in range(2):
            for e in range(2):
                for kxp, kx in ((1, e + 1 - 2 * b), (2, 3 + e - 2 * b), (0, e - 1 - 2 * b)):
                    if 0 <= kx <= 2:
                        w3[b, :cin, e, :, :, kxp] = w[:, :, :, kx]
        return w3.view(64, 32, 3, 3)

    @property
    def bias(self):
        return None if self.src.bias is None else torch.cat([self.src.bias.detach(), self.src.bias.detach()], 0)


class PackedOneHot:
    """Gather table [49][cin][64 | 128] of a 7x7 stem Conv2d (csrc/onehot_stem.hip), refreshed like PackedConv."""

    def __init__(self, eng, mod, slice_, T, label_nc):
        self.mod = mod
        self.cout, self.cin = mod.weight.shape[0], mod.weight.shape[1]
        self.dtype, self.slice, self.T, self.label_nc = eng.dtype, slice_, T, label_nc
        n = lib.v2v_onehot_conv_table_bytes(self.cin, self.cout, self.dtype, slice_, T, label_nc)
        if n <= 0:
            raise RuntimeError("onehot_conv_table_bytes(%d, %d) failed" % (self.cin, self.cout))
        self.buf = torch.empty(n, dtype=torch.uint8, device=eng.device)
        self.bias = None
        self.version = None
        self.refresh()

    def refresh(self, force=False):
        w = self.mod.weight
        box = getattr(w, "_v2v_epoch", None)
        ver = (w._version, w.data_ptr(), None if self.mod.bias is None else self.mod.bias._version, _PARAM_EPOCH[0],
               0 if box is None else box[0])
        if not force and ver == self.version:
            return
        w32 = w.detach()
        if w32.dtype != torch.float32 or not w32.is_contiguous():
            w32 = w32.float().contiguous()
        check(lib.v2v_onehot_conv_pack_weights(_ptr(w32), _ptr(self.buf), self.cin, self.cout, self.dtype, self.slice,
                                               self.T, self.label_nc, _stream()),
              "onehot_conv_pack_weights")
        self.bias = None if self.mod.bias is None else self.mod.bias.detach().float().contiguous()
        self.version = ver


class Plan:
    """Recorded launch sequence (v2v_plan) with optional hipGraph replay."""

    def __init__(self):
        self.h = C.c_void_p(lib.v2v_plan_create())
        self.keep = []          # tensors the recorded launches point into
        self.graph_ready = False

    def __enter__(self):
        check(lib.v2v_plan_begin_record(self.h), "plan_begin_record")
        return self

    def __exit__(self, *exc):
        check(lib.v2v_plan_end_record(self.h), "plan_end_record")
        return False

    def label(self, text):
        lib.v2v_plan_set_label(self.h, text.encode())

    @property
    def num_ops(self):
        return lib.v2v_plan_num_ops(self.h)

    def run(self):
        check(lib.v2v_plan_run(self.h, _stream()), "plan_run")

    def instantiate_graph(self):
        check(lib.v2v_plan_instantiate_graph(self.h, _stream()), "plan_instantiate_graph")
        self.graph_ready = True

    def launch(self):
        if self.graph_ready:
            check(lib.v2v_plan_launch_graph(self.h, _stream()), "plan_launch_graph")
        else:
            self.run()

    def profile(self):
        n = self.num_ops
        ms = (C.c_float * n)()
        check(lib.v2v_plan_profile(self.h, _stream(), ms, n), "plan_profile")
        out = []
        for i in range(n):
            out.append((lib.v2v_plan_op_name(self.h, i).decode(), lib.v2v_plan_op_label(self.h, i).decode(), ms[i]))
        return out

    def timeline(self, graph=True):
        """[(op, label, lane, start_ms, end_ms)] of one replay with every lane on its own stream: captured as a hipGraph
        (the real schedule) or issued eagerly (shows the host's issue order as well)."""
        n = self.num_ops
        t0, t1, ln = (C.c_float * n)(), (C.c_float * n)(), (C.c_int32 * n)()
        fn = lib.v2v_plan_timeline_graph if graph else lib.v2v_plan_timeline
        check(fn(self.h, _stream(), t0, t1, ln, n), "plan_timeline")
        return [(lib.v2v_plan_op_name(self.h, i).decode(), lib.v2v_plan_op_label(self.h, i).decode(), int(ln[i]), t0[i], t1[i])
                for i in range(n)]

    def __del__(self):
        try:
            lib.v2v_plan_destroy(self.h)
        except Exception:
            pass


FUSE_FINALIZE_MAX_PIXELS = 32768   # larger layers leave thousands of statistics rows: parallel two-stage finalize instead
PREFETCH_DIST = 12          # K chunks (128 B of every weight row each) the helper wave runs ahead


# Ticket words of one (lane, scratch set): [0, 256) the conv kernels' per-channel-tile arrive / depart tickets, [256, 256 + 64 * 128)
# the row-group tickets of the two-level in-kernel finalize (conv_igemm_kernel.h: fin_counter + 256 + g * n_tiles + nt), then the
# one-hot stems' per-slice tickets (onehot_stem.hip: fin_counter + blockIdx.y) in a region of their own (they used to
# start at word 256, inside the row-group region -- safe only while launches of one lane are serialised).
FIN_ONEHOT_OFFSET = 256 + 64 * 128
FIN_TAG_OFFSET = FIN_ONEHOT_OFFSET + 256            # include/v2v_hip.h V2V_FIN_TAG_WORD: the fused-norm launches' per-channel-tile launch tags
FIN_COUNTER_WORDS = FIN_TAG_OFFSET + 128


class Engine:
    """Emits v2v_* launches for one device / one activation dtype."""

    def __init__(self, device, dtype=L.F32, align_corners=False, record_only=False, x3=False):
        self.device = torch.device(device)
        # x3 (fp32 engine only): 3x3 convolutions whose input channels are whole 128-byte chunks run on the bf16 matrix pipe
        # over bf16x3 operands (X3Conv / split_x3): fp32-grade products at 3x the bf16 cost instead of the fp32-input MFMA
        # rate; statistics, norms, activations and everything else stay fp32
        self.x3 = bool(x3) and dtype == L.F32
        self._x3_engine = None
        self._x3_convs = {}
        # record_only: launches may only be RECORDED into a Plan (never executed).  Used by the CPU
        # test-suite to check the lowering (layer census, argument validation) without a GPU.
        self.record_only = record_only
        if self.device.type != "cuda" and not record_only:
            raise RuntimeError("vid2vid_amd runs on MI355X only (got device %s); there is no CPU path" % device)
        if record_only:
            # dry run: every v2v_* call still validates its arguments, nothing is ever launched (include/v2v_hip.h,
            # v2v_set_dry_run) -- lets the CPU test-suite drive whole training / inference control flows
            lib.v2v_set_dry_run(1)
        elif lib.v2v_get_dry_run():
            # the dry-run switch is process-wide: with it set, every launch, plan run and optimizer step of THIS engine
            # would return success without executing anything -- refuse instead of computing nothing
            raise RuntimeError("v2v dry-run mode is on (a record-only Engine was created in this process): call "
                               "vid2vid_amd.networks.set_record_only(False) before creating a GPU engine")
        self.dtype = dtype
        self.tdtype = _TORCH_DTYPE[dtype]
        self.align_corners = align_corners
        self._packed = {}        # id(module) -> PackedConv
        self._label_cmaps = {}   # label_nc -> uint8 (label_nc, 3) palette on the device (label_image)
        self._packed_onehot = {} # id(module) -> PackedOneHot (7x7 stems fed by label maps)
        # stems over encoded label maps as a weight gather-sum (csrc/onehot_stem.hip); V2V_ONEHOT_STEM=0: dense conv on the encoding
        self.onehot_stem = bool(int(os.environ.get("V2V_ONEHOT_STEM", "1")))
        self.onehot_slice = int(os.environ.get("V2V_ONEHOT_SLICE", "0"))      # output channels per workgroup: 32 / 64, 0 = default
        # conv + norm + activation + residuals in one launch (spin barrier between the workgroups of a channel tile) for
        # the paired ResnetBlock convolutions; V2V_FUSED_NORM=0: raw fp32 output + bn_apply launch
        self.fused_norm = bool(int(os.environ.get("V2V_FUSED_NORM", "1")))
        # V2V_RAW_BF16=1 (bf16 storage, inference plans): the pre-norm output of an UNPAIRED convolution (stride-2 / transposed stages,
        # the foreground tower, fine-scale ResnetBlocks) is stored as bf16 instead of fp32 (V2V_OUT_RAW_ACT_NHWC) -- the conv writes and
        # the bn_apply reads half the bytes; the statistics still come from the fp32 accumulators.  Built, tested
        # (test_conv_raw_output_in_activation_dtype) and measured on one box (profiles/r04_a6_raw_bf16_ab.txt): bn_apply -7 % / -10 %,
        # but the convolutions' epilogues pay more for the bf16 packing than the stores save (+3 % / +7 % conv time) -- the frame is
        # 1.7 % SLOWER at both resolutions and the bf16 error grows (fake_B mean 1.44e-2 -> 1.64e-2).  OFF by default.
        self.raw_bf16 = bool(int(os.environ.get("V2V_RAW_BF16", "0")))
        self.raw_bf16_one = os.environ.get("V2V_RAW_BF16_ONE", "1") != "0"      # bf16 raw output of the persistent single-chunk tiles (Engine.conv)
        # V2V_HEAD_ROWSUM=0: the bf16 generator heads (7x7, <= 4 output channels, planar fp32) stay on conv7x7_head_kernel (tile 60)
        # instead of conv7x7_rowsum_kernel (tile 62: row GEMM over (kernel column, channel) + shifted sum) -- A/B switch
        self.rowsum_heads = bool(int(os.environ.get("V2V_HEAD_ROWSUM", "1")))
        self._fused_norm_wgs = None
        # model_final_flow + model_final_w (same input) as one 7x7 head launch; V2V_MERGE_HEADS=0: one launch each
        self.merge_heads = bool(int(os.environ.get("V2V_MERGE_HEADS", "1")))
        self._merged_heads = {}
        self._scratch = {}       # name -> tensor (grown on demand, shared between layers)
        self._grids = {}
        self._zero_page = None
        self._fin_counters = {}   # per plan lane: concurrent branches must not share ticket words
        self._sk_counters = {}
        self._lane = 0           # current plan lane (hipGraph branch); selects the scratch set
        self._sset = 0           # scratch sub-set inside a lane: member 1 of a paired launch owns its own raw / stats / tickets
        # set by a multi-stream frame plan (B > 1 sequences per replay): every norm group of the launches emitted
        # meanwhile takes per-sample statistics -- nn.BatchNorm2d (training mode at batch 1 = per-sample statistics with affine
        # parameters) as well as nn.InstanceNorm2d -- from the conv epilogue's rows where each row belongs to one sample
        self.per_stream = False
        self.last_rows_per_sample = 0    # of the last conv() with statistics rows while per_stream: rows of one sample, or 0
        self.twin_enabled = False    # set by the frame plan: twin chains (label / image towers, image / flow branches) as paired launches
        self.pair_override = None    # (tile, splitk) forced for every paired launch (experiments: V2V_PAIR_TILE="70,1")
        if os.environ.get("V2V_PAIR_TILE"):
            self.pair_override = tuple(int(v) for v in os.environ["V2V_PAIR_TILE"].split(","))
        self.lanes_enabled = False   # set by the frame plan: emit independent towers / branches on parallel lanes
        self._thrash = None          # 384 MB the tile searches clear in front of every timed launch (_time_launch)
        self.pair_tune_log = {}      # pair key -> [(us, tile, splitk)] of its search, fastest first (experiments read it)
        # Round 6: weight-gradient launches of a backward pass go to a SIDE stream (autograd.ConvFn.backward).  dW is a leaf of
        # the backward graph -- nothing downstream of a layer's backward needs it before the optimizer step -- while the chain
        # norm-backward -> backward-data -> next layer is strictly serial and leaves the chip idle between its ~4000 dependent
        # launches per chunk (the device is busy 70 % of a chunk, and replaying the chunk as ONE hipGraph does not change that:
        # the gaps are the device's kernel-to-kernel turnaround, not host time; profiles/r06_v3_traingraph.txt).  V2V_WGRAD_STREAM=0
        # keeps everything on one stream.
        self.wgrad_stream_on = os.environ.get("V2V_WGRAD_STREAM", "1") != "0"
        self._wgrad_stream = None
        self._wgrad_join_queued = False
        self.repack_async_on = os.environ.get("V2V_REPACK_ASYNC", "1") != "0"
        self._repack_event = None
        import weakref
        _ENGINES.append(weakref.ref(self))
        self.plan = None        # Plan being recorded (for labels / keep-alive)
        self.conv_log = []       # (label, desc summary) of every conv emitted; used by bench/roofline
        self.tile_override = {}  # (cin,cout,KH,stride,transposed) -> tile id (tests / manual tuning)
        # V2V_TILE_OVERRIDE="cin,cout,K,stride,transposed:tile,splitk,prefetch;..." pins configurations (experiments)
        for item in os.environ.get("V2V_TILE_OVERRIDE", "").split(";"):
            if ":" in item:
                k, v = item.split(":")
                self.tile_override[tuple(int(x) for x in k.split(","))] = tuple(int(x) for x in v.split(","))
        self.autotune = False    # measure the tile configurations once per conv shape (plan build time)
        self._tuned = {}         # (cin,cout,KH,stride,transposed,N,H,W,out_mode,Cs) -> (tile, splitk, prefetch)
        self.bwd_tile_override = {}   # (dY channels, dX channels, KH, stride, transposed) of a backward-data operator -> tile (tests)
        self._tune_alts = {}     # same key -> runner-up configurations of the isolated search (this process only)
        self._tune_wide = {}     # same key -> the wider candidate list used for the heaviest shapes of a frame
        # optional persistent tuning cache (V2V_TUNE_CACHE=<json>): a profiling run can replay exactly the
        # configurations a previous benchmark run selected instead of re-measuring them under the profiler
        self._tune_cache_path = os.environ.get("V2V_TUNE_CACHE", "")
        if self._tune_cache_path and os.path.exists(self._tune_cache_path):
            try:
                with open(self._tune_cache_path) as f:
                    for k, v in json.load(f).get(str(dtype), {}).items():
                        self._tuned[tuple(int(x) for x in k.split(","))] = tuple(v)
            except (OSError, ValueError):
                pass
        self.update_running_stats = False
        self.fused_finalize = True   # norm statistics finalized by the conv kernel's last workgroup (small layers)
        # round 4, V2V_FIN2=1: layers with more than 512 statistics rows (> 32768 output pixels) finalize in the conv launch too, in
        # two levels (v2v_conv_desc.fin_workspace; bit for bit v2v_bn_finalize: test_two_level_in_kernel_finalize_equals_bn_finalize).
        # Built, tested, measured on one box (profiles/r04_b7_fin2_ab.txt): 66 launches fewer per 2048x1024 frame (355 -> 289), the
        # two finalize kernels -0.45 ms, but every workgroup of those thousand-tile launches now drains its stores and takes a ticket
        # before it exits: conv +1.0 ms -- 83.1 -> 80.3 frames/s (512x256: 372 -> 367).  OFF by default.
        self.fused_finalize2 = bool(int(os.environ.get("V2V_FIN2", "0")))
        self.last_finalized = False  # did the last conv() finalize its statistics in-kernel?
        self.ablate = 0              # profiling ablations (scripts/conv_ablate.py); results are wrong when set

    # ---------------- buffers ----------------
    def empty_act(self, N, H, W, C):
        t = torch.empty((N, H, W, pad_channels(C, self.dtype)), dtype=self.tdtype, device=self.device)
        self._keep(t)
        return Act(t, C)

    def zeros_act(self, N, H, W, C):
        a = self.empty_act(N, H, W, C)
        a.t.zero_()
        return a

    def empty_f32(self, *shape):
        t = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._keep(t)
        return t

    def scratch(self, name, numel, dtype=torch.float32, zero=False):
        """Shared scratch (conv raw output, statistics): consumed by the next launch on the
        same stream, so one buffer per kind is enough.  zero: the buffer starts as zeros (every time it is (re)allocated)."""
        key = (name, dtype, self._lane, self._sset)
        t = self._scratch.get(key)
        if t is None or t.numel() < numel:
            if self.plan is not None and t is not None and not self.record_only:
                raise RuntimeError("scratch '%s' must not grow while a plan is recording" % name)
            t = (torch.zeros if zero else torch.empty)(int(numel), dtype=dtype, device=self.device)
            self._scratch[key] = t
        self._keep(t)
        return t

    def reserve_scratch(self, raw_elems, stats_elems):
        self.scratch("raw", raw_elems)
        self.scratch("stats", stats_elems)

    def _keep(self, t):
        if self.plan is not None:
            self.plan.keep.append(t)

    def label(self, text):
        if self.plan is not None:
            self.plan.label(text)

    @property
    def _sk_counter(self):       # lane-0 split-K ticket words (tests check that kernels re-arm them)
        return self._sk_counters.get((0, 0))

    @property
    def _fin_counter(self):
        return self._fin_counters.get((0, 0))

    @contextlib.contextmanager
    def scratch_set(self, k):
        """Scratch sub-set k of the current lane (raw conv output, statistics, tickets, split-K slabs): the second member
        of a paired launch must not share them with the first."""
        prev, self._sset = self._sset, k
        try:
            yield
        finally:
            self._sset = prev

    # ---------------- plan lanes (parallel hipGraph branches) ----------------
    @contextlib.contextmanager
    def on_lane(self, k):
        """Emit the enclosed launches on plan lane k: a branch that starts after everything emitted so far on the
        current lane and runs concurrently with what the current lane emits next (include/v2v_hip.h, v2v_plan_set_lane).
        Each lane has its own scratch set / ticket words.  Without `lanes_enabled` this is a no-op."""
        parent = self._lane
        if not self.lanes_enabled or k == parent:
            yield
            return
        check(lib.v2v_plan_lane_wait(k, parent), "plan_lane_wait")       # fork
        self._lane = k
        check(lib.v2v_plan_set_lane(k), "plan_set_lane")
        try:
            yield
        finally:
            self._lane = parent
            check(lib.v2v_plan_set_lane(parent), "plan_set_lane")

    def join(self, k):
        """The current lane continues after everything emitted so far on lane k."""
        if self.lanes_enabled and k != self._lane:
            check(lib.v2v_plan_lane_wait(self._lane, k), "plan_lane_wait")

    def wgrad_side_stream(self):
        """The stream weight-gradient kernels run on, or None (switch off / no device / record-only engine)."""
        if not self.wgrad_stream_on or self.record_only or self.device.type != "cuda":
            return None
        if self._wgrad_stream is None:
            self._wgrad_stream = torch.cuda.Stream(device=self.device)
            from . import parallel
            parallel.register_grad_stream(self._wgrad_stream)      # bucket all-reduces sent from inside the pass must wait for it too
        return self._wgrad_stream

    def queue_wgrad_join(self):
        """Called from inside a backward pass after the first side-stream launch: when the autograd engine has finished the pass,
        the stream that called backward() waits for the side stream -- whatever reads .grad next (optimizer step, a test, a
        gradient clip) is ordered behind every weight-gradient kernel without knowing about the side stream."""
        if self._wgrad_join_queued:
            return
        self._wgrad_join_queued = True
        side = self._wgrad_stream

        def join():
            self._wgrad_join_queued = False
            torch.cuda.current_stream(self.device).wait_stream(side)
        torch.autograd.Variable._execution_engine.queue_callback(join)

    def face_window(self, real_A, openpose, crop_h, crop_w, name="face_win"):
        """v2v_face_window of planar fp32 real_A (N, C, H, W) into this engine's int32[8] buffer `name`:
        {found, ys, ye, xs, xe} of Vid2VidModelD.get_face_region (reference models/vid2vid_model_D.py:215-230), on the
        device -- no host read, no allocation after the first call.  The buffer is rewritten by the next call with the
        same name; the window packs of a discriminator pass (autograd.pack_concat_window) read it in their backward."""
        real_A = real_A.contiguous().float()
        N, Cc, H, W = real_A.shape
        win = self.scratch(name, L.FACE_WIN_WORDS, dtype=torch.int32, zero=True)
        mode = L.FACE_OPENPOSE if openpose else L.FACE_DENSEPOSE
        check(lib.v2v_face_window(_ptr(real_A), N, Cc, H, W, mode, crop_h, crop_w, _ptr(win), _stream()), "face_window")
        return win

    def zero_page(self):
        """256 zero bytes: source of padded / ragged lanes of the LDS-DMA loaders."""
        if self._zero_page is None:
            self._zero_page = torch.zeros(256, dtype=torch.uint8, device=self.device)
        return self._zero_page

    def grid(self, H, W):
        """Base sampling grid of get_grid (models/networks.py:79-93): torch.linspace(-1,1,n)."""
        key = (H, W)
        if key not in self._grids:
            gx = torch.linspace(-1.0, 1.0, W).to(self.device)
            gy = torch.linspace(-1.0, 1.0, H).to(self.device)
            self._grids[key] = (gx, gy)
        return self._grids[key]

    # ---------------- weights ----------------
    def packed(self, mod, cin_stride, role="fwd", reflect=False, korder=0, refresh=True, touch=True):
        """touch=False: the caller only wants the layer's geometry -- the packing is not marked as in use (repack_async re-packs
        after every optimizer step what was used since the last one: a patch-tile layer's tap-major packing, fetched by Engine.conv
        for its geometry and never read by a launch, was a third of those re-packs)."""
        key = (id(mod), cin_stride, role, reflect, korder)
        if self._repack_event is not None:
            self.wait_repack()    # packings refreshed on the side stream after the last optimizer step: this stream reads them from here on
        pc = self._packed.get(key)
        if pc is None:
            pc = PackedConv(self, mod, cin_stride, role, reflect, korder)
            self._packed[key] = pc
            pc.used = touch
        elif self.plan is None and refresh:
            pc.refresh()          # eager (training) use: follow optimizer updates
        if touch:
            pc.used = True
        return pc

    def repack_async(self, flat=None):
        """Refresh the stale packings of `flat`'s parameters that were used since the last call, on the side stream (see
        repack_after_step).  Packings whose owner is unknown (parameters re-homed after the packing was made, composed views) are
        left to the lazy refresh in front of their next use."""
        side = self.wgrad_side_stream()
        if side is None or self.plan is not None or not self.repack_async_on or torch.cuda.is_current_stream_capturing():
            return
        fid = id(flat) if flat is not None else None
        todo = [pc for pc in self._packed.values() if pc.used and (fid is None or pc.flat_id == fid)]
        if not todo:
            return
        cur = torch.cuda.current_stream(self.device)
        side.wait_stream(cur)                       # behind the optimizer kernel (and every reader of the old packings)
        with torch.cuda.stream(side):
            for pc in todo:
                pc.used = False
                pc.refresh()
            ev = torch.cuda.Event()
            ev.record(side)
        self._repack_event = ev

    def wait_repack(self):
        ev = self._repack_event
        if ev is not None:
            self._repack_event = None
            torch.cuda.current_stream(self.device).wait_event(ev)

    def refresh_weights(self, force=False):
        for pc in self._packed.values():
            pc.refresh(force)
        for pc in self._packed_onehot.values():
            pc.refresh(force)
        if self._x3_engine is not None:                 # the bf16x3 weight views live in the sub-engine (X3Conv.version_key follows the source layer)
            self._x3_engine.refresh_weights(force)

    # ---------------- one-hot stem (label-map input) ----------------
    def onehot_conv_ok(self, conv, cin, H, W, pad_mode=L.PAD_REFLECT, pad=3):
        """A 7x7 / stride 1 / ReflectionPad2d(3) Conv2d that can run as the gather-sum on label maps (inference only)."""
        return (self.onehot_stem and isinstance(conv, nn.Conv2d) and conv.kernel_size == (7, 7)
                and conv.stride == (1, 1) and conv.groups == 1 and pad_mode == L.PAD_REFLECT and pad == 3
                and conv.out_channels <= 128 and conv.in_channels == cin and H >= 4 and W >= 4
                and not (self.plan is None and torch.is_grad_enabled()))

    def onehot_eligible(self, x, conv, pad_mode, pad_override):
        """... straight on an encoded label Act."""
        # (N > 1: the batched stem of a multi-stream plan, staged from the codes of the batched frame prologue)
        return (x.onehot is not None and (x.N == 1 or (self.per_stream and x.onehot.codes is not None))
                and self.onehot_conv_ok(conv, x.C, x.H, x.W, pad_mode, conv.padding[0] if pad_override is None else pad_override))

    def label_codes(self, src, H, W):
        """One byte per (frame, pixel): label | instance-edge << 7 (v2v_label_codes), shared by every stem of the frame."""
        if src.label_nc > 126:
            return None
        codes = torch.empty((src.T, H, W), dtype=torch.uint8, device=self.device)
        self._keep(codes)
        check(lib.v2v_label_codes(_ptr(src.labels), _ptr(src.inst), int(src.labels.dtype == torch.uint8), _ptr(codes), src.T, H, W,
                                  src.label_nc, _stream()), "label_codes")
        self.label("label_codes")
        src.codes = codes
        return codes

    def frame_prologue(self, src, H, W, fg_labels, want_mask, window=None, last_C=0, row_slot=None):
        """Head of an inference frame whose label stems all run as gather-sums, in one launch (v2v_frame_prologue): the codes of
        label_codes, the foreground mask of encode_labels and -- with `window`, planar fp32 (1, C, H, W) -- the NHWC pack of the
        previous-frame window plus an fp32 copy of its last `last_C` planes (the warp's gather source).  The one-hot encoding
        is neither allocated nor written: the returned Act has its shape (a meta tensor) and its LabelSource, which is all a
        gather-sum stem reads.  Returns (x0, mask, packed Act or None, last or None).
        row_slot: int32 (N,) device tensor read by the launch when it runs (v2v_frame_prologue_pool; pool plans):
        `window` is then the pool (S, C, H, W) and dense row n packs and copies from slot row_slot[n]."""
        labels, inst, T = src.labels, src.inst, src.T
        N = labels.shape[0] if labels.dim() == 4 else 1      # multi-stream plans: maps (N, T, H, W), window (N, C, H, W)
        u8 = labels.dtype == torch.uint8
        if u8 and inst is not None and inst.dtype != torch.int32:
            raise TypeError("uint8 label maps go with int32 instance maps")
        if not u8 and (labels.dtype != torch.float32 or (inst is not None and inst.dtype != torch.float32)):
            raise TypeError("label / instance maps must be fp32-encoded integers, or uint8 + int32")
        if row_slot is not None:
            if (window is None or window.dim() != 4 or window.dtype != torch.float32 or not window.is_contiguous()
                    or row_slot.dtype != torch.int32 or tuple(row_slot.shape) != (N,) or not row_slot.is_contiguous()):
                raise ValueError("frame_prologue: a pooled head reads an fp32 pool (S, C, H, W) through int32 row_slot (N,)")
            self._keep(row_slot)
        elif N > 1 and window is not None and window.shape[0] != N:
            raise ValueError("frame_prologue: %d label streams, window of %d" % (N, window.shape[0]))
        per = src.label_nc + (1 if inst is not None else 0)
        codes = torch.empty((T, H, W) if N == 1 else (N, T, H, W), dtype=torch.uint8, device=self.device)
        self._keep(codes)
        mask = self.empty_f32(N, 1, H, W) if want_mask else None
        fg = None
        if want_mask:
            fg = self._fg_labels(fg_labels)
            self._keep(fg)
        packed = last = None
        win_C = cs = 0
        if window is not None:
            win_C = window.shape[1]
            packed = self.empty_act(N, H, W, win_C)
            cs = packed.Cs
            if last_C:
                last = self.empty_f32(N, last_C, H, W)
        # one sample is the batch entry point with N = 1 (what v2v_frame_prologue itself calls); the pool's takes S and row_slot
        # behind the window
        entry, pool = ("frame_prologue_batch", ()) if row_slot is None else ("frame_prologue_pool", (window.shape[0], _ptr(row_slot)))
        check(getattr(lib, "v2v_" + entry)(_ptr(labels), _ptr(inst), int(u8), _ptr(codes), _ptr(mask), _ptr(fg),
                                           0 if fg is None else fg.numel(), N, T, H, W, src.label_nc, _ptr(window), *pool, win_C,
                                           _ptr(None if packed is None else packed.t), cs, _ptr(last), last_C, self.dtype,
                                           _stream()), entry)
        self.label("frame_prologue")
        src.codes = codes
        x0 = Act(torch.empty((N, H, W, pad_channels(T * per, self.dtype)), dtype=self.tdtype, device="meta"), T * per, onehot=src)
        return x0, mask, packed, last

    def image_prologue(self, win, lut, window=None, last_C=0, advance=True, slot_mode=None, row_slot=None, pooled_window=False):
        """Head of an inference frame whose inputs are 8-bit images, in one launch (v2v_image_prologue).  win: the
        input window, uint8 (N, T, H, W, Cin), oldest frame first; lut: fp32 (Cin, 256), the decoded value of every byte of every
        channel.  Returns (x0, real_last, packed Act or None, last or None): x0 the NHWC stem input, channel t * Cin + c =
        lut[c][win[n, t, y, x, c]], bit for bit Engine.pack of the decoded planes; real_last fp32 (N, Cin, H, W), the newest
        frame as x0 holds it (Engine.unpack of its channels: the decoded values, bf16-rounded in a bf16 engine); with `window`, planar fp32 (N, C, H, W), its NHWC pack and an fp32 copy of its last `last_C` planes as
        Engine.frame_prologue returns them.  advance: the launch also moves the window on by a frame, win[:, t] <- win[:, t + 1]
        (slot T - 1 is left as it is), so the caller stages only the newest frame before the next launch.
        slot_mode, row_slot (v2v_image_prologue_slots): int32 (N,) device tensors read by the launch when it runs.
        slot_mode[n] == 2: row n is idle, its input window is not advanced (its outputs are written from it as it is).  row_slot:
        `win` is then the pool (S, T, H, W, Cin), dense row n works in place on win[row_slot[n]], and the results have N =
        row_slot.numel() rows; with pooled_window `window` is the fp32 pool (S, C, H, W) and row n packs window[row_slot[n]],
        without it `window` is dense (N, C, H, W)."""
        if not isinstance(win, torch.Tensor) or win.dtype != torch.uint8:
            raise TypeError("image_prologue: the input window is uint8 (N, T, H, W, Cin)")
        if not isinstance(lut, torch.Tensor) or lut.dtype != torch.float32:
            raise TypeError("image_prologue: the table is fp32 (Cin, 256)")
        if win.dim() != 5 or not win.is_contiguous():
            raise ValueError("image_prologue: the input window is contiguous uint8 (N, T, H, W, Cin)")
        N, T, H, W, Cin = win.shape
        S_win = S_window = 0
        if row_slot is not None:
            if (not isinstance(row_slot, torch.Tensor) or row_slot.dtype != torch.int32 or row_slot.dim() != 1
                    or not 1 <= row_slot.numel() <= N or not row_slot.is_contiguous() or row_slot.device != win.device):
                raise ValueError("image_prologue: a pooled head reads a uint8 pool (S, T, H, W, Cin) through int32 row_slot (N,), N <= S")
            S_win, N = N, row_slot.numel()
        elif pooled_window:
            raise ValueError("image_prologue: a pooled generated-frame window goes with row_slot")
        if slot_mode is not None and (not isinstance(slot_mode, torch.Tensor) or slot_mode.dtype != torch.int32
                                      or tuple(slot_mode.shape) != (N,) or not slot_mode.is_contiguous()
                                      or slot_mode.device != win.device):
            raise ValueError("image_prologue: slot_mode is int32 (%d,) on the window's device" % N)
        if Cin > 32:
            raise ValueError("image_prologue: %d input channels; the table of at most 32 channels is held in LDS" % Cin)
        if tuple(lut.shape) != (Cin, 256) or not lut.is_contiguous() or lut.device != win.device:
            raise ValueError("image_prologue: the table is contiguous fp32 (%d, 256) on the window's device, got %s"
                             % (Cin, tuple(lut.shape)))
        if window is not None:
            if window.dtype != torch.float32:
                raise TypeError("image_prologue: the generated-frame window is fp32 (N, C, H, W)")
            if pooled_window:
                if window.dim() != 4 or window.shape[0] < N or tuple(window.shape[2:]) != (H, W) or not window.is_contiguous():
                    raise ValueError("image_prologue: %d rows at %dx%d, pooled window %s" % (N, W, H, tuple(window.shape)))
                S_window = window.shape[0]
            elif window.dim() != 4 or tuple(window.shape[::3]) != (N, W) or window.shape[2] != H or not window.is_contiguous():
                raise ValueError("image_prologue: %d image streams at %dx%d, window %s" % (N, W, H, tuple(window.shape)))
            if not 0 <= last_C <= window.shape[1]:
                raise ValueError("image_prologue: last_C = %d of a window of %d planes" % (last_C, window.shape[1]))
        self._keep(win)
        self._keep(lut)
        x0 = self.empty_act(N, H, W, T * Cin)
        real_last = self.empty_f32(N, Cin, H, W)
        packed = last = None
        win_C = cs = 0
        if window is not None:
            self._keep(window)
            win_C = window.shape[1]
            packed = self.empty_act(N, H, W, win_C)
            cs = packed.Cs
            if last_C:
                last = self.empty_f32(N, last_C, H, W)
        elif pooled_window:
            raise ValueError("image_prologue: pooled_window without a window")
        # calls without words are the plain entry, unchanged; the slots entry takes the words and the pool sizes behind the stream
        entry, words = "image_prologue", ()
        if slot_mode is not None or row_slot is not None:
            for t in (slot_mode, row_slot):
                if t is not None:
                    self._keep(t)
            entry, words = "image_prologue_slots", (_ptr(slot_mode), _ptr(row_slot), S_win, S_window)
        check(getattr(lib, "v2v_" + entry)(_ptr(win), _ptr(lut), int(bool(advance)), _ptr(x0.t), x0.Cs, _ptr(real_last), N, T, H, W,
                                           Cin, _ptr(window), win_C, _ptr(None if packed is None else packed.t), cs, _ptr(last),
                                           last_C, self.dtype, _stream(), *words), entry)
        self.label("image_prologue")
        return x0, real_last, packed, last

    def gather_frames_u8(self, src, dst, entries, geoms):
        """uint8 frames at source size into uint8 frames at model size in one launch (v2v_gather_frames_u8): the
        loaders' nearest resize, crop and flip as an integer index map.  src: contiguous uint8 (..., Hs, Ws, C), its leading
        dimensions taken together as F frames; dst: contiguous uint8 (..., H, W, C), D frames -- e.g. a plan's or the pool's
        input windows (B, T, H, W, C).  entries: int32 (E, 4) = [src_frame, dst_frame, geom, 0]; geoms: int32 (G, 8) =
        [new_w, new_h, x1, y1, flip, 0, 0, 0] (visual.geometry_words); both in device memory, read when the launch runs, so
        inside a recorded plan (op "gather_frames_u8") a replay serves whatever the tables then hold.  Frames that no entry names
        are not written; an entry out of range does nothing.  E == 0 launches nothing."""
        for t, what in ((src, "src"), (dst, "dst")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
                raise TypeError("gather_frames_u8: %s is uint8 (..., rows, columns, C)" % what)
            if t.dim() < 3 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("gather_frames_u8: %s is contiguous uint8 (..., rows, columns, C) on the engine's device" % what)
        for t, what, cols in ((entries, "entries", 4), (geoms, "geoms", 8)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != cols
                    or not t.is_contiguous() or t.device != self.device or t.data_ptr() % 16 != 0):
                raise ValueError("gather_frames_u8: %s is contiguous int32 (n, %d) on the engine's device, 16-byte aligned" % (what, cols))
        Hs, Ws, Cc = src.shape[-3:]
        H, W = dst.shape[-3:-1]
        if dst.shape[-1] != Cc or not 1 <= Cc <= 32:
            raise ValueError("gather_frames_u8: src and dst have the same 1..32 channels, got %d and %d" % (Cc, dst.shape[-1]))
        if max(Hs, Ws, H, W) > 16384 or min(Hs, Ws, H, W) < 1 or geoms.shape[0] < 1 or entries.shape[0] > 65535:
            raise ValueError("gather_frames_u8: frames of 1..16384 rows and columns, at least one geometry, at most 65535 entries")
        if entries.shape[0] == 0:
            return
        F, D = src.numel() // (Hs * Ws * Cc), dst.numel() // (H * W * Cc)
        for t in (src, dst, entries, geoms):
            self._keep(t)
        check(lib.v2v_gather_frames_u8(_ptr(src), F, Hs, Ws, _ptr(dst), D, H, W, Cc, _ptr(entries), entries.shape[0],
                                       _ptr(geoms), geoms.shape[0], _stream()), "gather_frames_u8")
        self.label("gather_frames_u8")

    def onehot_conv(self, x, conv, want_stats=True, label="", fin=None):
        """Raw fp32 NHWC output + statistics rows of the stem convolution, computed from the label maps behind `x`.
        Returns (raw, rows, (N, OH, OW)) like conv(..., OUT_RAW_F32_NHWC, want_stats=True).  fin = (norm, ss): the
        statistics are finalized in the kernel (last workgroup of each channel slice), no bn_finalize launch."""
        src = x.onehot
        pk = self._packed_onehot.get((id(conv), self.onehot_slice))
        if pk is None:
            pk = self._packed_onehot[(id(conv), self.onehot_slice)] = PackedOneHot(self, conv, self.onehot_slice, src.T, src.label_nc)
        elif self.plan is None:
            pk.refresh()
        H, W, cout, N = x.H, x.W, conv.out_channels, x.N
        cs = (cout + 3) // 4 * 4
        raw = self.scratch("raw", N * H * W * cs)
        rows = N * lib.v2v_onehot_conv_stats_rows(H, W) if want_stats else 0      # sample-major: rows // N per sample
        st = self.scratch("stats", rows * cout * 2) if want_stats else None
        self._keep(pk.buf)
        if pk.bias is not None:
            self._keep(pk.bias)
        if src.codes is not None:
            lab_ptr, in_mode = _ptr(src.codes), 2
        else:
            lab_ptr, in_mode = _ptr(src.labels), int(src.labels.dtype == torch.uint8)
        if N > 1:
            if fin is not None or src.codes is None:
                raise RuntimeError("the batched gather-sum stem stages from the codes and has no in-kernel (batch-wide) finalize")
            check(lib.v2v_onehot_conv7x7_batch(lab_ptr, _ptr(src.inst), in_mode, _ptr(pk.buf), _ptr(pk.bias), _ptr(raw), _ptr(st),
                                               N, src.T, H, W, src.label_nc, cout, cs, self.dtype, pk.slice, _stream()),
                  "onehot_conv7x7_batch " + label)
        elif fin is not None and want_stats:
            norm, ss = fin
            gamma, beta, eps, mom, rm, rv = self._norm_params(norm, 1)
            key = (self._lane, self._sset)
            fin_counter = self._fin_counters.get(key)
            if fin_counter is None:
                fin_counter = self._fin_counters[key] = torch.zeros(FIN_COUNTER_WORDS, dtype=torch.int32, device=self.device)
            fn = L.OneHotNorm()          # (not _attach_finalize: another struct -- v2v_onehot_norm, no fin_ prefix -- and ticket words of its own)
            fn.counter = fin_counter.data_ptr() + 4 * FIN_ONEHOT_OFFSET  # own region: clear of the conv kernels' per-tile tickets (0..255) AND of the two-level finalize's row-group tickets (256 .. 256 + 64*128)
            fn.gamma = None if gamma is None else gamma.data_ptr()
            fn.beta = None if beta is None else beta.data_ptr()
            fn.scale_shift = ss.data_ptr()
            fn.running_mean = None if rm is None else rm.data_ptr()
            fn.running_var = None if rv is None else rv.data_ptr()
            fn.eps, fn.momentum, fn.count = eps, mom, H * W
            for t in (gamma, beta, ss, fin_counter):
                if t is not None:
                    self._keep(t)
            check(lib.v2v_onehot_conv7x7_norm(lab_ptr, _ptr(src.inst), in_mode, _ptr(pk.buf),
                                              _ptr(pk.bias), _ptr(raw), _ptr(st), src.T, H, W, src.label_nc, cout, cs, self.dtype,
                                              pk.slice, C.byref(fn), _stream()), "onehot_conv7x7_norm " + label)
        else:
            check(lib.v2v_onehot_conv7x7(lab_ptr, _ptr(src.inst), in_mode, _ptr(pk.buf),
                                         _ptr(pk.bias), _ptr(raw), _ptr(st), src.T, H, W, src.label_nc, cout, cs, self.dtype,
                                         pk.slice, _stream()), "onehot_conv7x7 " + label)
        self.label(label)
        if len(self.conv_log) >= 100000:
            del self.conv_log[:]
        # flops: those of the dense convolution this launch replaces (the frame's nominal 2115 GFLOP census), flagged
        self.conv_log.append(dict(label=label, N=N, H=H, W=W, OH=H, OW=W, cin=conv.in_channels, cout=cout, tune_key=None,
                                  KH=7, KW=7, stride=1, transposed=False, onehot=True,
                                  flops=2.0 * N * H * W * cout * conv.in_channels * 49, tile=(0, 0), splitk=1, prefetch=0))
        return raw, rows, (N, H, W)

    # ---------------- primitive emitters ----------------
    def conv(self, x, mod, pad_mode=L.PAD_ZERO, pad_override=None, out_mode=L.OUT_RAW_F32_NHWC,
             act=L.ACT_NONE, act_param=0.0, out_scale=1.0, want_stats=False, out=None, label="", fin=None, act_b=None, raw_act_ok=False):
        """Emit one convolution.  Returns (out, stats_rows, (N,OH,OW)).
        fin = (norm module, ss tensor [4*cout]): finalize the training-mode norm statistics inside the conv
        kernel (last-arriving workgroup), so no separate bn_finalize launch is needed."""
        pc = self.packed(mod, x.Cs, refresh=False, touch=False)     # geometry now; the packing that the chosen tile reads is fetched (and refreshed) below
        pad = pc.pad if pad_override is None else pad_override
        N, H, W = x.N, x.H, x.W
        if pc.transposed:
            OH = (H - 1) * pc.stride - 2 * pad + pc.KH + pc.out_pad
            OW = (W - 1) * pc.stride - 2 * pad + pc.KW + pc.out_pad
        else:
            OH = (H + 2 * pad - pc.KH) // pc.stride + 1
            OW = (W + 2 * pad - pc.KW) // pc.stride + 1
        d = self._desc_common(x, pc, pad, pad_mode, OH, OW)
        # raw_act_ok (conv_group -> norm_apply only): the raw tensor may be stored in the activation dtype.  Never on the autograd
        # path (the backward kernels read fp32 raw), never for the 7x7 layers (tiles 60 / 61 and the gather-sum stems write fp32)
        raw_ok_t = bool(raw_act_ok and out_mode == L.OUT_RAW_F32_NHWC and self.dtype == L.BF16 and out is None
                        and pc.KH != 7 and not torch.is_grad_enabled())
        raw_t = raw_ok_t and self.raw_bf16
        d.out_mode, d.act = (L.OUT_RAW_ACT_NHWC if raw_t else out_mode), act
        d.act_param, d.out_scale = act_param, out_scale
        if act_b is not None:          # (first channel, activation, parameter, scale) of the second head of a merged pair
            d.act_split, d.act_b, d.act_param_b, d.out_scale_b = act_b
        d.tile, d.splitk, d.prefetch = _cfg3(self.tile_override.get((pc.cin, pc.cout, pc.KH, pc.stride, int(pc.transposed)), 0))
        tune_key = (pc.cin, pc.cout, pc.KH, pc.stride, int(pc.transposed), N, H, W, out_mode, x.Cs)
        if d.tile == 0 and tune_key in self._tuned:
            d.tile, d.splitk, d.prefetch = _cfg3(self._tuned[tune_key])
        if raw_ok_t and not raw_t and self.raw_bf16_one and d.tile in PERSISTENT_TILES:
            # round 6: the persistent single-chunk tiles write their raw output rounded to bf16 (the statistics come from the fp32
            # accumulators): these layers are HBM-bound and the raw tensor is written once and read once by bn_apply -- 4 instead of
            # 8 bytes per element for the pair.  V2V_RAW_BF16_ONE=0 keeps fp32 raw.
            raw_t = True
            d.out_mode = L.OUT_RAW_ACT_NHWC
        if d.tile in PERSISTENT_TILES and not (self.dtype == L.BF16 and d.out_mode in (L.OUT_RAW_F32_NHWC, L.OUT_RAW_ACT_NHWC)):
            # a cached / overridden selection made under another raw-output mode or dtype (the key holds the LOGICAL out_mode:
            # V2V_RAW_BF16 flips the effective one; an fp32 engine may share the cache file): the persistent tiles write fp32 raw
            # from bf16 only -- fall back to the library's default tile instead of failing at launch
            d.tile, d.splitk, d.prefetch = 0, 1, 0
        if act_b is not None:
            d.tile, d.splitk, d.prefetch = HEAD_TILE, 1, 0   # per-channel epilogues exist in the 7x7 head kernels only
        if d.tile == HEAD_TILE and self.rowsum_heads and (pc.cin, pc.cout, pc.KH, pc.stride, int(pc.transposed)) not in self.tile_override \
                and self.dtype == L.BF16 and pc.cout <= 4 and out_mode == L.OUT_F32_NCHW \
                and x.Cs % 32 == 0 and not want_stats and fin is None:
            d.tile = ROWSUM_TILE                              # conv7x7_rowsum_kernel: the heads as row GEMM + shifted sum (bf16)
        if tile_korder(d.tile):
            pc = self._use_korder(d, mod, x.Cs, tile_korder(d.tile))
        else:
            pc.used = True             # this launch reads the tap-major packing
            if self.plan is None:
                pc.refresh()           # eager use: follow optimizer updates (only the packing this launch reads)
        d.bias = None if pc.bias is None else pc.bias.data_ptr()      # of the packing in use (aliases the parameter)
        if pc.cin != x.C:
            raise RuntimeError("conv %s: input has %d channels, layer expects %d" % (label, x.C, pc.cin))
        if raw_t:
            cs = (pc.cout + 7) // 8 * 8
            d.cout_stride = cs
            out = self.scratch("raw", (N * OH * OW * cs + 1) // 2)[:N * OH * OW * cs // 2].view(torch.bfloat16)     # the same scratch, half the bytes
            d.out = out.data_ptr()
        elif out_mode == L.OUT_RAW_F32_NHWC:
            cs = (pc.cout + 3) // 4 * 4
            d.cout_stride = cs
            if out is None:
                out = self.scratch("raw", N * OH * OW * cs)
            d.out = out.data_ptr()
        elif out_mode == L.OUT_ACT_NHWC:
            if out is None:
                out = self.empty_act(N, OH, OW, pc.cout)
                if out.Cs != pc.cout:
                    out.t.zero_()          # padded channels must read as zero downstream
            d.cout_stride = out.Cs
            d.out = out.t.data_ptr()
        else:
            if out is None:
                out = self.empty_f32(N, pc.cout, OH, OW)
            d.cout_stride = pc.cout
            d.out = out.data_ptr()
        rows = 0
        if want_stats:
            d.stats = None
            rows = lib.v2v_conv_stats_rows(C.byref(d))
            if rows <= 0:
                check(rows or -1, "conv_stats_rows")
            st = self.scratch("stats", rows * pc.cout * 2)
            d.stats = st.data_ptr()
            # (not for the 7x7 layers: their halo-patch tiles 60 / 61 have no in-kernel finalize and must stay eligible)
            two_level = bool(fin is not None and N * OH * OW > FUSE_FINALIZE_MAX_PIXELS and self.fused_finalize2 and rows > 512
                             and pc.KH != 7 and d.tile not in (HEAD_TILE, C8_TILE))
            if fin is not None and N * OH * OW > FUSE_FINALIZE_MAX_PIXELS and not two_level and not (d.tile in PERSISTENT_TILES and ONE_FIN):
                fin = None             # one workgroup walking >1000 rows costs 0.1-1 ms (profiles/r01_v15_finalize_tail.txt)
                                       # (the persistent tiles leave one row per WORKGROUP, <= 256: they finalize in the launch at any size)
            self.last_finalized = fin is not None
            if fin is not None:
                self._attach_finalize(d, fin[0], fin[1], N, N * OH * OW)
                if two_level:          # round 4: large layers finalize inside the conv launch in two levels (no bn_partial_reduce / bn_finalize launches)
                    d.fin_workspace = self.scratch("bn_ws", 64 * pc.cout * 2, torch.float64).data_ptr()
        if pc.bias is not None:
            self._keep(pc.bias)
        if (self.autotune and d.tile == 0 and self.plan is None and not self.record_only
                and not torch.is_grad_enabled()):
            self._tuned[tune_key], self._tune_alts[tune_key], self._tune_wide[tune_key] = self._autotune(d, want_stats, pc.cout, mod, x.Cs)
            self._save_tune_cache()
            d.tile, d.splitk, d.prefetch = self._tuned[tune_key]
            pc = self._use_korder(d, mod, x.Cs, tile_korder(d.tile))
            d.bias = None if pc.bias is None else pc.bias.data_ptr()
            if want_stats:
                rows = lib.v2v_conv_stats_rows(C.byref(d))
                d.stats = self.scratch("stats", rows * pc.cout * 2).data_ptr()
        self._splitk_workspace(d)
        self._keep(pc.buf)
        if self.per_stream:
            self.last_rows_per_sample = max(int(lib.v2v_conv_stats_rows_per_sample(C.byref(d))), 0) if want_stats else 0
        check(lib.v2v_conv2d(C.byref(d), _stream()), "conv2d " + label)
        self.label(label)
        ntaps = pc.KH * pc.KW
        if len(self.conv_log) >= 100000:          # eager (training) use without a consumer: keep the log bounded
            del self.conv_log[:]
        self.conv_log.append(dict(label=label, N=N, H=H, W=W, OH=OH, OW=OW, cin=pc.cin, cout=pc.cout, tune_key=tune_key,
                                  KH=pc.KH, KW=pc.KW, stride=pc.stride, transposed=pc.transposed,
                                  flops=2.0 * N * (H * W if pc.transposed else OH * OW) * pc.cout * pc.cin * ntaps,
                                  tile=lib.v2v_conv_tile_config(C.byref(d)), splitk=max(int(d.splitk), 1),
                                  prefetch=int(d.prefetch), convs=2 if act_b is not None else 1))    # merged heads: two reference layers
        return out, rows, (N, OH, OW)

    def _desc_common(self, x, pc, pad, pad_mode, OH, OW):
        """What every conv descriptor says: operands, geometry (that of packing `pc`), no split-K; raw fp32 NHWC output without
        activation until the caller says otherwise."""
        d = ConvDesc()
        d.in_ = x.t.data_ptr(); d.w = pc.buf.data_ptr(); d.w_korder = pc.korder
        d.zero_page = self.zero_page().data_ptr()
        self._keep(self._zero_page)
        d.bias = None if pc.bias is None else pc.bias.data_ptr()
        d.N, d.H, d.W = x.N, x.H, x.W
        d.cin, d.cin_stride, d.cout = pc.cin, x.Cs, pc.cout
        d.KH, d.KW, d.stride, d.pad, d.pad_mode = pc.KH, pc.KW, pc.stride, pad, pad_mode
        d.transposed = int(pc.transposed)
        d.OH, d.OW = OH, OW
        d.dtype, d.out_mode, d.act = self.dtype, L.OUT_RAW_F32_NHWC, L.ACT_NONE
        d.act_param, d.out_scale = 0.0, 1.0
        d.ablate = self.ablate
        return d

    def _attach_finalize(self, d, norm, ss, N, count):
        """The launch finalizes its statistics over `count` pixels itself (last-arriving workgroup): `ss` receives [4][C] scale /
        shift / mean / invstd of training-mode `norm`.  The ticket words are one buffer per (lane, scratch set)."""
        gamma, beta, eps, mom, rm, rv = self._batchwide_params(norm, N)
        key = (self._lane, self._sset)
        fin_counter = self._fin_counters.get(key)
        if fin_counter is None:
            fin_counter = self._fin_counters[key] = torch.zeros(FIN_COUNTER_WORDS, dtype=torch.int32, device=self.device)
        d.fin_counter = fin_counter.data_ptr()
        d.fin_gamma = None if gamma is None else gamma.data_ptr()
        d.fin_beta = None if beta is None else beta.data_ptr()
        d.fin_scale_shift = ss.data_ptr()
        d.fin_running_mean = None if rm is None else rm.data_ptr()
        d.fin_running_var = None if rv is None else rv.data_ptr()
        d.fin_eps, d.fin_momentum, d.fin_count = eps, mom, count
        for t in (gamma, beta, ss, fin_counter):
            if t is not None:
                self._keep(t)

    def _bn_finalize(self, rows, cout, count, norm, ss, N, label):
        """The statistics rows a conv launch left in the "stats" scratch -> `ss`, as a launch of its own (two-stage above 512 rows)."""
        gamma, beta, eps, mom, rm, rv = self._batchwide_params(norm, N)
        st = self.scratch("stats", rows * cout * 2)
        for t in (gamma, beta):
            if t is not None:
                self._keep(t)
        groups = lib.v2v_bn_finalize_groups(rows)
        ws = self.scratch("bn_ws", groups * cout * 2, torch.float64) if groups > 0 else None
        check(lib.v2v_bn_finalize(_ptr(st), rows, cout, count, _ptr(gamma), _ptr(beta), eps,
                                  _ptr(ss), _ptr(rm), _ptr(rv), mom, _ptr(ws), _stream()), "bn_finalize " + label)
        self.label(label + ".norm")

    # ---------------- paired launches (twin chains) ----------------
    def pair_eligible(self, xa, ma, xb, mb):
        """Can two 3x3 / stride 1 / pad 1 convolutions run as ONE v2v_conv2d_pair launch?  Identical geometry, channel
        stride a whole 128-byte chunk (the LDS-patch kernels' requirement), both behind a training-mode norm."""
        if self._training() or not isinstance(ma, nn.Conv2d) or not isinstance(mb, nn.Conv2d):
            return False
        bke = 64 if self.dtype == L.BF16 else 32
        same = (ma.in_channels == mb.in_channels and ma.out_channels == mb.out_channels and ma.kernel_size == mb.kernel_size
                and ma.stride == mb.stride and (ma.bias is None) == (mb.bias is None)
                and tuple(xa.t.shape) == tuple(xb.t.shape) and xa.Cs == xb.Cs and xa.C == xb.C)
        return bool(same and ma.kernel_size == (3, 3) and ma.stride == (1, 1) and xa.Cs % bke == 0)

    def _pair_desc(self, x, mod, pad_mode, pad, tile3, fin, label, fused=None):
        """Descriptor of one member of a paired launch: raw fp32 NHWC output + statistics (+ in-kernel finalize) on the
        CURRENT scratch sub-set.  fused = (act, act_param, res0, res1, y): the norm, activation and residual adds run in
        the conv kernel (V2V_OUT_NORM_ACT_NHWC) and `y` (an Act) receives the result; no raw tensor."""
        pc = self.packed(mod, x.Cs, korder=1, refresh=False)       # the channel-chunk-major packing every pair tile reads
        if self.plan is None:
            pc.refresh()
        N, H, W = x.N, x.H, x.W
        d = self._desc_common(x, pc, pad, pad_mode, H, W)         # (pair_eligible: 3x3 / stride 1 Conv2d)
        d.tile, d.splitk, d.prefetch = tile3
        if pc.cin != x.C:
            raise RuntimeError("conv %s: input has %d channels, layer expects %d" % (label, x.C, pc.cin))
        cs = (pc.cout + 3) // 4 * 4
        d.cout_stride = cs
        if fused is not None:
            act, act_param, res0, res1, y = fused
            raw = None
            d.out_mode, d.act, d.act_param = L.OUT_NORM_ACT_NHWC, act, act_param
            d.cout_stride = y.Cs
            d.out = y.t.data_ptr()
            d.res0 = None if res0 is None else res0.t.data_ptr()
            d.res1 = None if res1 is None else res1.t.data_ptr()
        else:
            raw = self.scratch("raw", N * H * W * cs)
            d.out = raw.data_ptr()
        d.stats = None
        rows = lib.v2v_conv_stats_rows(C.byref(d))
        if rows <= 0:
            check(rows or -1, "conv_stats_rows")
        if fused is not None:
            # tagged statistics granules (include/v2v_hip.h, "fused norm"): a zero-initialised buffer that only fused launches write
            d.stats = self.scratch("stats_tagged", rows * pc.cout * 4, zero=True).data_ptr()
        else:
            d.stats = self.scratch("stats", rows * pc.cout * 2).data_ptr()
        finalized = fin is not None and (fused is not None or N * H * W <= FUSE_FINALIZE_MAX_PIXELS)
        if finalized:
            self._attach_finalize(d, fin[0], fin[1], N, N * H * W)
        if pc.bias is not None:
            self._keep(pc.bias)
        if not self._splitk_workspace(d):
            raise RuntimeError("conv pair %s: split-K %d does not fit this layer" % (label, tile3[1]))
        self._keep(pc.buf)
        return d, raw, rows, finalized, pc

    def fused_norm_fits(self, tile3, N, H, W, cout, members=2):
        """V2V_OUT_NORM_ACT_NHWC (include/v2v_hip.h, "fused norm"): single-phase tiles, no split-K, every workgroup of the
        launch resident at once."""
        t, S = tile3[0], max(int(tile3[1]), 1)
        if not (self.fused_norm and self.fused_finalize and (_flag(t, L.TILE_FUSED_NORM) or t in EXP_TILES) and S == 1 and cout % vec_of(self.dtype) == 0):
            return False
        th, tw, bn = PATCH_CFGS[t]
        if self._fused_norm_wgs is None:
            self._fused_norm_wgs = int(lib.v2v_conv_fused_norm_max_workgroups())
        return members * N * -(-H // th) * -(-W // tw) * -(-cout // bn) <= self._fused_norm_wgs

    # ---------------- bf16x3 ("x3") operands for the fp32 engine ----------------
    def _x3_ok(self, x, conv, pad_override=None, with_norm=True):
        tr = isinstance(conv, nn.ConvTranspose2d)
        if not (self.x3 and (isinstance(conv, nn.Conv2d) or (tr and tuple(conv.stride) == (2, 2))) and conv.groups == 1
                and conv.kernel_size in ((3, 3), (7, 7)) and x.C == conv.in_channels and x.C % 64 == 0 and x.Cs == x.C
                and self.fused_finalize and not self._training() and not self.record_only):
            return False
        if not with_norm:
            return True
        pad = conv.padding[0] if pad_override is None else pad_override
        st, k = conv.stride[0], conv.kernel_size[0]
        if tr:
            OH, OW = (x.H - 1) * st - 2 * pad + k + conv.output_padding[0], (x.W - 1) * st - 2 * pad + k + conv.output_padding[0]
        else:
            OH, OW = (x.H + 2 * pad - k) // st + 1, (x.W + 2 * pad - k) // st + 1
        return x.N * OH * OW <= FUSE_FINALIZE_MAX_PIXELS          # the statistics are finalized inside the conv launch

    def _x3_enter(self):
        sub = self._x3_engine
        if sub is None:
            sub = self._x3_engine = Engine(self.device, L.BF16, self.align_corners)
            sub.fused_norm = False                                # the norm runs in fp32 on the raw output (bn_apply of THIS engine)
        sub.plan, sub._lane, sub._sset = self.plan, self._lane, self._sset
        sub.autotune, sub.update_running_stats, sub.lanes_enabled = self.autotune, self.update_running_stats, self.lanes_enabled
        sub.fused_finalize = self.fused_finalize
        return sub

    def _x3_wrap(self, conv):
        w = self._x3_convs.get(id(conv))
        if w is None:
            w = self._x3_convs[id(conv)] = X3Conv(conv)
        return w

    def _x3_out(self, y):
        """The bf16x3 side output of a bn_apply that produces `y`, or None when `y` cannot feed an x3 convolution."""
        if not (self.x3 and y.C % 64 == 0 and y.Cs == y.C and not self._training() and not self.record_only):
            return None
        t = torch.empty((y.N, y.H, y.W, 3 * y.C), dtype=torch.bfloat16, device=self.device)
        self._keep(t)
        y.x3 = Act(t, 3 * y.C)
        return t

    def split_x3(self, x):
        """fp32 Act (C channels, C % 64 == 0, dense stride) -> bf16 Act of 3 C channels [hi | lo | hi]."""
        if x.x3 is not None:                                      # written by the producing bn_apply (v2v_bn_apply_x3)
            return x.x3
        out = torch.empty((x.N, x.H, x.W, 3 * x.C), dtype=torch.bfloat16, device=self.device)
        self._keep(out)
        check(lib.v2v_split_x3(_ptr(x.t), _ptr(out), x.N * x.H * x.W, x.C, x.Cs, 3 * x.C, _stream()), "split_x3")
        self.label("split_x3")
        return Act(out, 3 * x.C)

    def _x3_log(self, sub, n0):
        for c in sub.conv_log[n0:]:                               # algorithmic work in this engine's census (K was tripled)
            self.conv_log.append(dict(c, cin=c["cin"] // 3, flops=c["flops"] / 3.0, x3=True))
        del sub.conv_log[n0:]

    def conv_pair(self, xa, ma, xb, mb, pad_mode, pad, fins, labels, fuse=None):
        """Two convolutions of identical geometry as ONE launch (include/v2v_hip.h, v2v_conv2d_pair).  Member b works on
        scratch sub-set 1 of the current lane.  Returns ((raw, rows, finalized), (raw, rows, finalized)), shape.
        fuse = (act, act_param, adds_a, adds_b, ya, yb): when the selected tile allows it the norm / activation /
        residual adds run inside the launch and ya / yb receive the results (raw is then None)."""
        N, H, W = xa.N, xa.H, xa.W
        key = (-2, ma.in_channels, ma.out_channels, N, H, W, xa.Cs)
        if self.pair_override is not None:
            tile3 = (self.pair_override[0], self.pair_override[1], 0)
        elif key in self._tuned:
            tile3 = _cfg3(self._tuned[key])
        elif self.autotune and self.plan is None and not self.record_only and not torch.is_grad_enabled():
            tile3 = self._tuned[key] = self._autotune_pair(xa, ma, xb, mb, pad_mode, pad, fins, key, fuse=fuse)
            self._save_tune_cache()
        else:
            tile3 = (TS.default_pair_tile(W), 1, 0)
        fa = fb = None
        if fuse is not None and fins[0] is not None and self.fused_norm_fits(tile3, N, H, W, ma.out_channels):
            act, act_param, adds_a, adds_b, ya, yb = fuse
            fa, fb = (act, act_param, adds_a[0], adds_a[1], ya), (act, act_param, adds_b[0], adds_b[1], yb)
        da, rawa, rowsa, fina, pca = self._pair_desc(xa, ma, pad_mode, pad, tile3, fins[0], labels[0], fused=fa)
        with self.scratch_set(1):
            db, rawb, rowsb, finb, pcb = self._pair_desc(xb, mb, pad_mode, pad, tile3, fins[1], labels[1], fused=fb)
        check(lib.v2v_conv2d_pair(C.byref(da), C.byref(db), _stream()), "conv2d_pair " + labels[0])
        self.label(labels[0] + " + " + labels[1])
        for lbl, pc in ((labels[0], pca), (labels[1], pcb)):
            self.conv_log.append(dict(label=lbl, N=N, H=H, W=W, OH=H, OW=W, cin=pc.cin, cout=pc.cout, tune_key=key,
                                      KH=3, KW=3, stride=1, transposed=False, pair=True, fused_norm=fa is not None,
                                      flops=2.0 * N * H * W * pc.cout * pc.cin * 9,
                                      tile=tile3[0], splitk=max(int(tile3[1]), 1), prefetch=0))
        return ((rawa, rowsa, fina), (rawb, rowsb, finb)), (N, H, W)

    def _autotune_pair(self, xa, ma, xb, mb, pad_mode, pad, fins, key, reps=7, fuse=None):
        """Measured choice of (tile, split-K) for a paired launch among tile_search.pair_candidates (cold weights, as _autotune)."""
        st = _stream()
        best, best_ms, alts = None, float("inf"), []
        for t, S, _ in TS.pair_candidates(xa.N, xa.H, xa.W, xa.Cs, ma.out_channels, self.dtype):
            fa = fb = None
            if fuse is not None and fins[0] is not None and self.fused_norm_fits((t, S, 0), xa.N, xa.H, xa.W, ma.out_channels):
                act, act_param, adds_a, adds_b, ya, yb = fuse         # timed as it will run: norm / act / adds in the launch
                fa, fb = (act, act_param, adds_a[0], adds_a[1], ya), (act, act_param, adds_b[0], adds_b[1], yb)
            try:
                da = self._pair_desc(xa, ma, pad_mode, pad, (t, S, 0), fins[0], "tune", fused=fa)[0]
                with self.scratch_set(1):
                    db = self._pair_desc(xb, mb, pad_mode, pad, (t, S, 0), fins[1], "tune", fused=fb)[0]
            except RuntimeError:
                continue
            ms = self._time_launch(lambda: lib.v2v_conv2d_pair(C.byref(da), C.byref(db), st), reps)
            if ms is None:
                continue
            if fuse is not None and fa is None:
                ms += 0.012                  # the bn_apply_pair launch the unfused variant still needs (~6 us + its gap)
            alts.append((ms, (t, S, 0)))
            if ms < best_ms:
                best, best_ms = (t, S, 0), ms
        if best is None:
            raise RuntimeError("no paired-launch tile fits this layer")
        alts.sort()
        self._tune_alts[key] = [c for _, c in alts if c != best][:5]
        self._tune_wide[key] = []
        self.pair_tune_log[key] = [(round(ms * 1e3, 1), c[0], c[1]) for ms, c in alts]
        return best

    def conv_group_pair(self, xa, conva, norma, xb, convb, normb, pad_mode, pad_override, act, act_param,
                        adds_a=(None, None), adds_b=(None, None), labels=("", "")):
        """Two [pad] conv + norm [+ act] [+ residuals] groups of identical geometry: ONE paired conv launch (statistics
        finalized in-kernel) + ONE paired normalise / activate / add launch.  Returns (Act a, Act b)."""
        cout = conva.out_channels
        ssa = self.scratch("scale_shift", 4 * cout)
        with self.scratch_set(1):
            ssb = self.scratch("scale_shift", 4 * cout)
        pad = conva.padding[0] if pad_override is None else pad_override
        fins = ((norma, ssa), (normb, ssb)) if self.fused_finalize else (None, None)
        N, OH, OW = xa.N, xa.H, xa.W
        ya, yb = self.empty_act(N, OH, OW, cout), self.empty_act(N, OH, OW, cout)
        if self._x3_ok(xa, conva, pad) and self._x3_ok(xb, convb, pad):
            sub = self._x3_enter()
            n0 = len(sub.conv_log)
            xa3 = self.split_x3(xa)
            with self.scratch_set(1):
                xb3 = self.split_x3(xb)
            (ra, rb), shp = sub.conv_pair(xa3, self._x3_wrap(conva), xb3, self._x3_wrap(convb), pad_mode, pad, fins, labels, fuse=None)
            self._x3_log(sub, n0)
        else:
            (ra, rb), shp = self.conv_pair(xa, conva, xb, convb, pad_mode, pad, fins, labels,
                                           fuse=(act, act_param, adds_a, adds_b, ya, yb))
        if ra[0] is None:                 # norm + activation + residuals ran inside the conv launch
            return ya, yb
        cs_raw = (cout + 3) // 4 * 4
        for (raw, rows, fin), norm, ss, k, lbl in ((ra, norma, ssa, 0, labels[0]), (rb, normb, ssb, 1, labels[1])):
            if not fin:                                       # large layers: parallel two-stage finalize per member
                with self.scratch_set(k):
                    self._bn_finalize(rows, cout, N * OH * OW, norm, ss, N, lbl)
        a0, a1 = adds_a
        b0, b1 = adds_b
        xa3, xb3 = self._x3_out(ya), self._x3_out(yb)
        if xa3 is not None and xb3 is not None:
            check(lib.v2v_bn_apply_x3(_ptr(ra[0]), _ptr(ssa), _ptr(None if a0 is None else a0.t), _ptr(None if a1 is None else a1.t), _ptr(ya.t), _ptr(xa3),
                                      _ptr(rb[0]), _ptr(ssb), _ptr(None if b0 is None else b0.t), _ptr(None if b1 is None else b1.t), _ptr(yb.t), _ptr(xb3),
                                      cs_raw, N * OH * OW, cout, act, act_param, _stream()), "bn_apply_x3 (pair) " + labels[0])
        else:
            check(lib.v2v_bn_apply_pair(_ptr(ra[0]), _ptr(ssa), _ptr(None if a0 is None else a0.t), _ptr(None if a1 is None else a1.t), _ptr(ya.t),
                                        _ptr(rb[0]), _ptr(ssb), _ptr(None if b0 is None else b0.t), _ptr(None if b1 is None else b1.t), _ptr(yb.t),
                                        cs_raw, N * OH * OW, cout, ya.Cs, act, act_param, self.dtype, _stream()),
                  "bn_apply_pair " + labels[0])
        self.label(labels[0] + ".apply + " + labels[1] + ".apply")
        return ya, yb

    def run_resblocks_twin(self, blocks_a, xa, blocks_b, xb, name_a, name_b, first_index=0):
        """Two chains of ResnetBlocks of identical shape (models/networks.py:554-593) in lock step: every convolution pair
        is one launch that fills the chip (csrc/conv3x3_pp2_kernel.h), every normalise / residual pair one launch.
        Falls back to two independent chains when the pair is not eligible."""
        blocks_a, blocks_b = list(blocks_a), list(blocks_b)
        assert len(blocks_a) == len(blocks_b)
        for k, (ba, bb) in enumerate(zip(blocks_a, blocks_b)):
            ma, mb = list(ba.conv_block), list(bb.conv_block)
            def take(mods, j):
                pad_mode, pad_override = L.PAD_ZERO, None
                if isinstance(mods[j], nn.ReflectionPad2d):
                    pad_mode, pad_override = L.PAD_REFLECT, int(mods[j].padding[0]); j += 1
                return pad_mode, pad_override, mods[j], mods[j + 1], j + 2
            pm, po, c1a, n1a, ja = take(ma, 0)
            _, _, c1b, n1b, jb = take(mb, 0)
            na, nb = "%s.%d" % (name_a, first_index + k), "%s.%d" % (name_b, first_index + k)
            # (per-sample InstanceNorm2d at batch > 1: the paired launches finalize batch-wide -> two independent chains)
            if not self.pair_eligible(xa, c1a, xb, c1b) or self.per_sample(n1a, xa.N) or self.per_sample(n1b, xb.N):
                xa = self.run_resblock(ba, xa, None, na)
                xb = self.run_resblock(bb, xb, None, nb)
                continue
            act, act_param = self._act_code(ma[ja]); ja += 1; jb += 1
            ha, hb = self.conv_group_pair(xa, c1a, n1a, xb, c1b, n1b, pm, po, act, act_param, labels=(na + ".c1", nb + ".c1"))
            pm, po, c2a, n2a, _ = take(ma, ja)
            _, _, c2b, n2b, _ = take(mb, jb)
            xa, xb = self.conv_group_pair(ha, c2a, n2a, hb, c2b, n2b, pm, po, L.ACT_NONE, 0.0,
                                          adds_a=(xa, None), adds_b=(xb, None), labels=(na + ".c2", nb + ".c2"))
        return xa, xb

    def tune_backward_data(self, d, dx_channels, conv=None, reflect=False):
        """Tile selection for a backward-data launch (autograd._conv_backward_data): same measured search as the
        forward convs (implicit-GEMM tiles x split-K; the operator is the forward kernel with role-swapped weights),
        keyed separately (leading -1) in the same tuning table.  Measured only while `autotune` is on (the first
        training steps of bench.py --mode train); later steps replay the selection."""
        key = (-1, d.cin, d.cout, d.KH, d.stride, d.transposed, d.N, d.H, d.W, d.cin_stride, d.cout_stride, d.pad)

        def use(cfg):                                # configuration, the packing its tile reads, its split-K workspace
            d.tile, d.splitk, d.prefetch = cfg
            if conv is not None:
                self._use_korder(d, conv, d.cin_stride, tile_korder(d.tile), role="bwd", reflect=reflect)
            return self._splitk_workspace(d)

        forced = self.bwd_tile_override.get((d.cin, d.cout, d.KH, d.stride, int(d.transposed)))
        if forced is not None:                       # tests: a given tile for the backward-data operator (dY channels, dX channels, k, stride, transposed)
            if not use(_cfg3(forced)):
                raise RuntimeError("bwd_tile_override: split-K workspace")
            return
        if key not in self._tuned:
            if not (self.autotune and self.plan is None and not self.record_only):
                use((0, 0, 0))
                return
            # conv given: the patch kernels are candidates too -- backward-data of a stride-2 Conv2d is a transposed stride-2 convolution
            # (conv3x3_t2_kernel), that of a ConvTranspose2d a stride-2 convolution (conv3x3_s2_kernel), on the role-swapped packings
            self._tuned[key], self._tune_alts[key], self._tune_wide[key] = self._autotune(
                d, False, dx_channels, mod=conv, cin_stride=d.cin_stride, role="bwd", reflect=reflect)
            self._save_tune_cache()
        if not use(_cfg3(self._tuned[key])):
            use((0, 0, 0))

    def log_backward(self, kind, label, conv, cin, cout, N, pixels):
        """Algorithmic FLOP of a backward launch (same count as its forward conv), for bench.py's training roofline."""
        if len(self.conv_log) < 100000:
            self.conv_log.append(dict(label=kind + ":" + label, kind=kind, cin=cin, cout=cout, KH=conv.kernel_size[0],
                                      KW=conv.kernel_size[1], N=N, tile=-1, splitk=1, prefetch=0,
                                      flops=2.0 * N * pixels * cout * cin * conv.kernel_size[0] * conv.kernel_size[1]))

    def _save_tune_cache(self):
        if not self._tune_cache_path:
            return
        data = {}
        if os.path.exists(self._tune_cache_path):
            try:
                with open(self._tune_cache_path) as f:
                    data = json.load(f)
            except (OSError, ValueError):
                data = {}
        data[str(self.dtype)] = {",".join(str(int(x)) for x in k): list(v) for k, v in self._tuned.items()}
        with open(self._tune_cache_path, "w") as f:
            json.dump(data, f)

    def _use_korder(self, d, mod, cin_stride, korder, role="fwd", reflect=False):
        if role == "bwd" and d.tile == C8_TILE:
            if not TS.bwd_c8_eligible(d, self.dtype, mod):
                raise ValueError("tile 61 as a backward-data operator: a 7x7 / stride 1 Conv2d whose output gradient is one 16-byte vector per pixel")
            pc = self.packed(mod, cin_stride, role="bwd", reflect=reflect, korder=5)
            d.transposed, d.pad = 0, pc.KH - 1 - pc.pad
            d.w, d.w_korder = pc.buf.data_ptr(), 0
            return pc
        if role == "bwd" and korder == 1 and _flag(d.tile, L.TILE_PAD2) and TS.bwd_patch_eligible(d, self.dtype, mod):
            pc = self.packed(mod, cin_stride, role="bwd", reflect=reflect, korder=4)
            d.transposed, d.pad = 0, pc.KH - 1 - pc.pad
            d.w, d.w_korder = pc.buf.data_ptr(), 1
            return pc
        if d.tile in PERSISTENT_TILES and cin_stride == 32 and role == "fwd" and (TS.pairx_eligible(d, self.dtype) or TS.pairx_t_eligible(d, self.dtype)):
            # 64-byte pixels on the persistent single-chunk tiles: paired-x packing (PairedXConv).  Gated on the view's own
            # eligibility (round 6: an fp32 engine's 32-channel layers -- one 128-byte chunk, patch-eligible, so the
            # persistent tiles are among the candidates -- took this branch and PairedXConv raised for FlowNet2's 64 -> 32
            # layers at 512x256); everything else keeps the tile's own packing and the library refuses what it cannot run
            korder = 3
        pc = self.packed(mod, cin_stride, role=role, reflect=reflect, korder=korder)
        d.w, d.w_korder = pc.buf.data_ptr(), korder
        if role == "bwd":
            d.transposed, d.pad = int(pc.transposed), pc.pad      # (a previous candidate may have been the convolution form above)
        return pc

    def _splitk_workspace(self, d):
        """Attach the split-K slab scratch and ticket words to a descriptor (no-op for splitk <= 1)."""
        if d.splitk <= 1:
            d.splitk = 0
            d.slabs = None
            d.sk_counter = None
            return True
        tickets = C.c_int32(0)
        nbytes = lib.v2v_conv_splitk_workspace(C.byref(d), C.byref(tickets))
        if nbytes <= 0:
            return False
        skc = self._sk_counters.get((self._lane, self._sset))
        if skc is None or skc.numel() < tickets.value:
            if self.plan is not None and not self.record_only and skc is not None:      # (a first buffer of this lane is safe: nothing recorded points at one yet)
                raise RuntimeError("split-K ticket buffer must not grow while a plan is recording")
            skc = self._sk_counters[(self._lane, self._sset)] = torch.zeros(max(4096, tickets.value), dtype=torch.int32, device=self.device)
        d.slabs = self.scratch("slabs", (nbytes + 3) // 4).data_ptr()
        d.sk_counter = skc.data_ptr()
        self._keep(skc)
        return True

    def _autotune(self, d, want_stats, cout, mod=None, cin_stride=0, role="fwd", reflect=False):
        """Time every (tile, split-K, weight-prefetch) configuration tile_search.conv_candidates lists for this launch; returns
        (fastest triple, runners-up, wider list: tile_search.runners_up).  Runs once per conv shape while a frame plan is being
        built, never inside a timed region."""
        cands = TS.conv_candidates(d, self.dtype, cout, mod, role, self.rowsum_heads)
        st = _stream()
        def prepare(t, S, pf):
            d.tile, d.splitk, d.prefetch = t, S, pf
            if mod is not None:
                self._use_korder(d, mod, cin_stride, tile_korder(t), role=role, reflect=reflect)
            if want_stats:
                rows = lib.v2v_conv_stats_rows(C.byref(d))
                if rows <= 0:
                    return False
                d.stats = self.scratch("stats", rows * cout * 2).data_ptr()
            return self._splitk_workspace(d)

        launch = lambda: lib.v2v_conv2d(C.byref(d), st)
        timed = []
        for cfg in cands:
            ms = self._time_launch(launch, 3, lambda: prepare(*cfg))
            if ms is not None:
                timed.append((ms, cfg))
        if os.environ.get("V2V_TUNE_DEBUG"):
            print("autotune %s: %d candidates, %d ran; fastest %s; last error: %s" % ((d.cin, d.cout, d.KH, d.stride, d.transposed, d.cout_stride), len(cands), len(timed),
                  sorted(timed)[:3], lib.v2v_last_error().decode()[:200]), file=sys.stderr)
        if not timed:
            return (0, 1, 0), [], []
        # second pass over the front-runners with more repetitions: single medians of 3 are noisy enough to flip
        # the choice between runs (181 vs 194 fps observed)
        timed.sort()
        best, best_ms = timed[0][1], float("inf")
        for _, cfg in timed[:6]:
            ms = self._time_launch(launch, 11, lambda: prepare(*cfg))
            if ms is not None and ms < best_ms:
                best, best_ms = cfg, ms
        return (best,) + TS.runners_up(timed, best)

    def _time_launch(self, launch, reps, prepare=None):
        """Median milliseconds of `reps` runs of launch() (a library call: 0 = launched), None when prepare() or the first launch
        refuses.  Each timed run follows a 384 MB memset: at batch 1 a frame streams ~0.8 GB of weights, so every layer meets
        its weights COLD in L2 / Infinity Cache -- back-to-back warm launches favour shallow LDS-DMA rings and no prefetch,
        which stall on real frames."""
        if self._thrash is None:
            self._thrash = torch.empty(96 << 20, dtype=torch.float32, device=self.device)
        if (prepare is not None and not prepare()) or launch() != 0:
            return None
        e0, e1 = ([torch.cuda.Event(enable_timing=True) for _ in range(reps)] for _ in range(2))
        for r in range(reps):
            self._thrash.zero_()
            e0[r].record()
            launch()
            e1[r].record()
        e1[-1].synchronize()
        return sorted(a.elapsed_time(b) for a, b in zip(e0, e1))[reps // 2]      # median

    def _norm_params(self, norm, N):
        """(gamma, beta, eps, momentum, running_mean, running_var) of a training-mode norm layer
        (get_norm_layer, models/networks.py:23-30; .eval() is never called in the reference)."""
        if isinstance(norm, nn.BatchNorm2d):
            gamma = norm.weight.detach() if norm.affine else None
            beta = norm.bias.detach() if norm.affine else None
            eps, mom = norm.eps, (norm.momentum if norm.momentum is not None else 0.1)
            rm = norm.running_mean if (self.update_running_stats and norm.track_running_stats) else None
            rv = norm.running_var if (self.update_running_stats and norm.track_running_stats) else None
            if rm is not None and self.plan is None:
                norm._v2v_batches = getattr(norm, "_v2v_batches", 0) + 1     # -> num_batches_tracked at save time
            return gamma, beta, eps, mom, rm, rv
        if isinstance(norm, nn.InstanceNorm2d):
            # N > 1: the caller takes per-sample statistics (inst_batched / inorm_apply); batch-wide finalize paths are not eligible
            gamma = norm.weight.detach() if norm.affine else None
            beta = norm.bias.detach() if norm.affine else None
            return gamma, beta, norm.eps, 0.1, None, None
        raise NotImplementedError("norm layer %r" % type(norm))

    @staticmethod
    def inst_batched(norm, N):
        """InstanceNorm2d at batch > 1: statistics per sample.  Such a group takes them from the conv's raw output
        (v2v_in_stats -> v2v_in_apply, csrc/instance_norm.hip) and is not eligible for any path that finalizes the
        statistics of the whole launch (fin=, fused-norm pair tiles, the persistent tiles' in-launch finalize)."""
        return isinstance(norm, nn.InstanceNorm2d) and N > 1

    def per_sample(self, norm, N):
        """inst_batched, or ANY norm layer at batch > 1 while a multi-stream inference plan is emitted (per_stream): the
        samples are independent sequences, each normalised as a batch-1 model would."""
        return self.inst_batched(norm, N) or (self.per_stream and N > 1 and isinstance(norm, (nn.BatchNorm2d, nn.InstanceNorm2d)))

    def _batchwide_params(self, norm, N):
        """_norm_params for a finalize over ALL N*OH*OW pixels of a launch: an error for a per-sample norm at batch > 1."""
        if self.per_sample(norm, N):
            raise RuntimeError("%s at batch %d reached a batch-wide statistics finalize (per-sample statistics needed)"
                               % (type(norm).__name__, N))
        return self._norm_params(norm, N)

    def _in_scratch(self, N, HW, cout):
        """(workspace, tickets) of the v2v_in_* launches on this lane / scratch sub-set (tickets start as zeros, re-armed in-kernel)."""
        ws = self.scratch("in_ws", (lib.v2v_in_workspace_bytes(HW, cout, N) + 7) // 8, torch.float64)
        tk = self.scratch("in_tickets", lib.v2v_in_ticket_words(cout, N), torch.int32, zero=True)
        return ws, tk

    def inorm_apply(self, raw, shape, cout, norm, act, act_param, add0=None, add1=None, label="", ss=None, rows_per_sample=0):
        """InstanceNorm2d at batch > 1 on the conv's raw NHWC output: v2v_in_stats (per-sample [N][4][C] scale / shift /
        mean / invstd into `ss`, kept by the caller for the backward pass on the training path) + v2v_in_apply.
        rows_per_sample > 0 (multi-stream plans): the conv launch left N * rows_per_sample statistics rows, sample-major, in
        the "stats" scratch -- v2v_in_finalize_rows reduces them instead of a second read of raw."""
        N, OH, OW = shape
        raw_dt = L.BF16 if raw.dtype == torch.bfloat16 else L.F32      # Engine.conv(raw_act_ok=True): V2V_OUT_RAW_ACT_NHWC
        cs_raw = (cout + 7) // 8 * 8 if raw_dt == L.BF16 else (cout + 3) // 4 * 4
        if ss is None:
            ss = self.scratch("in_scale_shift", N * 4 * cout)
        gamma, beta, eps, _, _, _ = self._norm_params(norm, N)
        for t in (gamma, beta, ss):
            if t is not None:
                self._keep(t)
        if rows_per_sample > 0:
            st = self.scratch("stats", N * rows_per_sample * cout * 2)
            nbytes = lib.v2v_in_finalize_rows_workspace(rows_per_sample, cout, N)
            ws = self.scratch("in_rows_ws", nbytes // 8, torch.float64) if nbytes > 0 else None
            check(lib.v2v_in_finalize_rows(_ptr(st), rows_per_sample, N, cout, OH * OW, _ptr(gamma), _ptr(beta), eps, _ptr(ss),
                                           _ptr(ws), _stream()), "in_finalize_rows " + label)
        else:
            ws, tk = self._in_scratch(N, OH * OW, cout)
            check(lib.v2v_in_stats(_ptr(raw), raw_dt, cs_raw, _ptr(gamma), _ptr(beta), eps, _ptr(ss), _ptr(ws), _ptr(tk),
                                   N, OH * OW, cout, _stream()), "in_stats " + label)
        self.label(label + ".norm")
        y = self.empty_act(N, OH, OW, cout)
        y3 = self._x3_out(y)
        check(lib.v2v_in_apply(_ptr(raw), raw_dt, cs_raw, _ptr(ss), _ptr(None if add0 is None else add0.t),
                               _ptr(None if add1 is None else add1.t), _ptr(y.t), _ptr(y3), N, OH * OW, cout, y.Cs,
                               act, act_param, self.dtype, _stream()), "in_apply " + label)
        self.label(label + ".apply")
        return y

    def norm_apply(self, raw, rows, shape, cout, norm, act, act_param, add0=None, add1=None, label="", ss=None,
                   finalized=False):
        """[bn_finalize +] bn_apply on the shared raw/statistics scratch (ss: caller-owned [4][C] statistics
        buffer, kept for the backward pass on the training path; finalized: the conv kernel already wrote it)."""
        N, OH, OW = shape
        raw_bf16 = raw.dtype == torch.bfloat16                 # Engine.conv(raw_act_ok=True): V2V_OUT_RAW_ACT_NHWC
        cs_raw = (cout + 7) // 8 * 8 if raw_bf16 else (cout + 3) // 4 * 4
        if ss is None:
            ss = self.scratch("scale_shift", 4 * cout)
        if not finalized:
            self._bn_finalize(rows, cout, N * OH * OW, norm, ss, N, label)
        y = self.empty_act(N, OH, OW, cout)
        y3 = self._x3_out(y)
        if y3 is not None:
            check(lib.v2v_bn_apply_x3(_ptr(raw), _ptr(ss), _ptr(None if add0 is None else add0.t), _ptr(None if add1 is None else add1.t),
                                      _ptr(y.t), _ptr(y3), None, None, None, None, None, None,
                                      cs_raw, N * OH * OW, cout, act, act_param, _stream()), "bn_apply_x3 " + label)
        elif raw_bf16:
            check(lib.v2v_bn_apply_raw(_ptr(raw), L.BF16, cs_raw, _ptr(ss),
                                       _ptr(None if add0 is None else add0.t), _ptr(None if add1 is None else add1.t),
                                       _ptr(y.t), N * OH * OW, cout, y.Cs, act, act_param, self.dtype, _stream()),
                  "bn_apply_raw " + label)
        else:
            check(lib.v2v_bn_apply(_ptr(raw), cs_raw, _ptr(ss),
                                   _ptr(None if add0 is None else add0.t), _ptr(None if add1 is None else add1.t),
                                   _ptr(y.t), N * OH * OW, cout, y.Cs, act, act_param, self.dtype, _stream()),
                  "bn_apply " + label)
        self.label(label + ".apply")
        return y

    def conv_group(self, x, conv, pad_mode, pad_override, norm, act, act_param, add0=None, add1=None,
                   head_nchw=False, out_scale=1.0, label=""):
        """One fused [pad] conv [norm] [act] [+ residuals] group.  Returns an Act, or the planar fp32 NCHW
        tensor when head_nchw.  With autograd recording on (training) it is a v2v custom op
        (autograd.ConvFn: same launches, tensors saved for the HIP backward kernels)."""
        if self.plan is None and torch.is_grad_enabled():
            from . import autograd as AG
            return AG.conv_group(self, x, conv, pad_mode, pad_override, norm, act, act_param, add0, add1,
                                 head_nchw, out_scale, label)
        if norm is not None and self.onehot_eligible(x, conv, pad_mode, pad_override) and self.per_sample(norm, x.N):
            # batched gather-sum stem: its tiles are cut per sample, every statistics row belongs to one stream
            raw, rows, shp = self.onehot_conv(x, conv, label=label)
            return self.inorm_apply(raw, shp, conv.out_channels, norm, act, act_param, add0=add0, add1=add1, label=label,
                                    rows_per_sample=rows // x.N)
        if norm is not None and self.onehot_eligible(x, conv, pad_mode, pad_override):
            ss = self.scratch("scale_shift", 4 * conv.out_channels)
            fin = (norm, ss) if self.fused_finalize else None
            raw, rows, shp = self.onehot_conv(x, conv, label=label, fin=fin)
            return self.norm_apply(raw, rows, shp, conv.out_channels, norm, act, act_param, add0=add0, add1=add1, label=label,
                                   ss=ss, finalized=fin is not None)
        if norm is not None and self.per_sample(norm, x.N):
            # per-sample statistics: the conv runs without statistics rows and without fin= (both are batch-wide)
            if self.per_stream and not self._x3_ok(x, conv, pad_override, with_norm=False):
                # multi-stream plan: statistics rows, no fin=; where every row belongs to one sample (tile table:
                # v2v_conv_stats_rows_per_sample) they are finalized per sample, else raw is read a second time (v2v_in_stats)
                raw, _, shp = self.conv(x, conv, pad_mode, pad_override, L.OUT_RAW_F32_NHWC, want_stats=True, label=label,
                                        raw_act_ok=True)
                return self.inorm_apply(raw, shp, conv.out_channels, norm, act, act_param, add0=add0, add1=add1, label=label,
                                        rows_per_sample=self.last_rows_per_sample)
            if self._x3_ok(x, conv, pad_override, with_norm=False):
                sub = self._x3_enter()
                n0 = len(sub.conv_log)
                raw, _, shp = sub.conv(self.split_x3(x), self._x3_wrap(conv), pad_mode, pad_override, L.OUT_RAW_F32_NHWC, label=label)
                self._x3_log(sub, n0)
            else:
                raw, _, shp = self.conv(x, conv, pad_mode, pad_override, L.OUT_RAW_F32_NHWC, label=label, raw_act_ok=True)
            return self.inorm_apply(raw, shp, conv.out_channels, norm, act, act_param, add0=add0, add1=add1, label=label)
        if norm is not None:
            ss = self.scratch("scale_shift", 4 * conv.out_channels)
            if self._x3_ok(x, conv, pad_override):
                sub = self._x3_enter()
                n0 = len(sub.conv_log)
                raw, rows, shp = sub.conv(self.split_x3(x), self._x3_wrap(conv), pad_mode, pad_override, L.OUT_RAW_F32_NHWC,
                                          want_stats=True, label=label, fin=(norm, ss))
                self.last_finalized = sub.last_finalized
                self._x3_log(sub, n0)
            else:
                raw, rows, shp = self.conv(x, conv, pad_mode, pad_override, L.OUT_RAW_F32_NHWC, want_stats=True, label=label,
                                           fin=(norm, ss) if self.fused_finalize else None, raw_act_ok=True)
            return self.norm_apply(raw, rows, shp, conv.out_channels, norm, act, act_param, add0=add0, add1=add1,
                                   label=label, ss=ss, finalized=self.fused_finalize and self.last_finalized)
        if add0 is not None or add1 is not None:
            raise NotImplementedError("residual adds need a norm layer in the group")
        bke = 32 if self.dtype == L.BF16 else 16              # the 7x7 head kernel reads whole 64-byte half chunks
        if (head_nchw and isinstance(conv, nn.Conv2d) and conv.kernel_size == (7, 7) and conv.out_channels <= 32
                and x.Cs % bke != 0 and x.H * x.W >= 65536):
            x = self.widen(x, (x.Cs + bke - 1) // bke * bke)      # e.g. the 16-channel foreground tower of scale 2: 32-byte rows
        if head_nchw and self._x3_ok(x, conv, pad_override, with_norm=False):     # API-facing 7x7 heads: planar fp32 straight from the bf16x3 product
            sub = self._x3_enter()
            n0 = len(sub.conv_log)
            out, _, _ = sub.conv(self.split_x3(x), self._x3_wrap(conv), pad_mode, pad_override, L.OUT_F32_NCHW, act, act_param, out_scale, label=label)
            self._x3_log(sub, n0)
            return out
        out, _, _ = self.conv(x, conv, pad_mode, pad_override, L.OUT_F32_NCHW if head_nchw else L.OUT_ACT_NHWC,
                              act, act_param, out_scale if head_nchw else 1.0, label=label)
        return out

    def head_pair(self, x, seq_a, scale_a, seq_b, scale_b, label=""):
        """Two API-facing heads on the same input ([ReflectionPad2d(3), Conv2d(C, n, 7) [, act]] each: model_final_flow and
        model_final_w, models/networks.py:181-183) as ONE launch writing one planar fp32 tensor; returns the two channel
        ranges as views.  None when the pair does not qualify (the caller then emits them one by one)."""
        def parse(seq):
            mods = list(seq)
            if not (len(mods) in (2, 3) and isinstance(mods[0], nn.ReflectionPad2d) and isinstance(mods[1], nn.Conv2d)):
                return None
            act = (L.ACT_NONE, 0.0) if len(mods) == 2 else self._act_code(mods[2])
            return None if act is None else (int(mods[0].padding[0]), mods[1], act)
        pa, pb = parse(seq_a), parse(seq_b)
        if (not self.merge_heads or self.x3 or pa is None or pb is None or self._training() or pa[0] != pb[0]
                or pa[1].kernel_size != (7, 7) or pa[1].out_channels + pb[1].out_channels > 16):
            return None
        key = (id(pa[1]), id(pb[1]))
        merged = self._merged_heads.get(key)
        if merged is None:
            try:
                merged = self._merged_heads[key] = MergedConv(pa[1], pb[1])
            except ValueError:
                return None
        bke = 32 if self.dtype == L.BF16 else 16
        if x.Cs % bke != 0:                       # the 7x7 head kernel reads whole 64-byte half chunks
            if x.H * x.W < 65536:
                return None
            x = self.widen(x, (x.Cs + bke - 1) // bke * bke)
        ca = pa[1].out_channels
        out, _, _ = self.conv(x, merged, L.PAD_REFLECT, pa[0], L.OUT_F32_NCHW, pa[2][0], pa[2][1], scale_a, label=label,
                              act_b=(ca, pb[2][0], pb[2][1], scale_b))
        return out[:, :ca], out[:, ca:]

    # ---------------- nn.Sequential lowering ----------------
    @staticmethod
    def _act_code(m):
        if isinstance(m, nn.ReLU): return L.ACT_RELU, 0.0
        if isinstance(m, nn.LeakyReLU): return L.ACT_LEAKY, float(m.negative_slope)
        if isinstance(m, nn.Tanh): return L.ACT_TANH, 0.0
        if isinstance(m, nn.Sigmoid): return L.ACT_SIGMOID, 0.0
        return None

    def run_sequential(self, seq, x, extra_add=None, head_nchw=False, out_scale=1.0, name="", collect=None, first_index=0):
        """Run an nn.Sequential (or list of modules) on Act `x`.

        extra_add: Act added to the output of the LAST stage (tower sums, coarse features).
        head_nchw: the last conv writes planar fp32 NCHW (API-facing heads).
        collect:   optional list receiving the output of every top-level module group
                   (MultiscaleDiscriminator.getIntermFeat).
        first_index: index of seq[0] inside the nn.Sequential it was sliced from (labels keep the reference's numbering).
        """
        mods = list(seq)
        i, n = 0, len(mods)
        while i < n:
            m = mods[i]
            last_group = False
            if isinstance(m, (nn.ReflectionPad2d, nn.Conv2d, nn.ConvTranspose2d)):
                pad_mode, pad_override = L.PAD_ZERO, None
                if isinstance(m, nn.ReflectionPad2d):
                    pad_mode, pad_override = L.PAD_REFLECT, int(m.padding[0])
                    i += 1
                    m = mods[i]
                    if not isinstance(m, nn.Conv2d) or m.padding[0] != 0:
                        raise NotImplementedError("ReflectionPad2d must be followed by an unpadded Conv2d")
                conv = m
                i += 1
                norm = None
                if i < n and isinstance(mods[i], (nn.BatchNorm2d, nn.InstanceNorm2d)):
                    norm = mods[i]; i += 1
                act, act_param = L.ACT_NONE, 0.0
                if i < n and self._act_code(mods[i]) is not None:
                    act, act_param = self._act_code(mods[i]); i += 1
                last_group = i >= n
                lbl = "%s.%d" % (name, first_index + i)
                if norm is not None:
                    x = self.conv_group(x, conv, pad_mode, pad_override, norm, act, act_param,
                                        add0=extra_add if last_group else None, label=lbl)
                    if last_group:
                        extra_add = None
                elif head_nchw and last_group:
                    return self.conv_group(x, conv, pad_mode, pad_override, None, act, act_param,
                                           head_nchw=True, out_scale=out_scale, label=lbl)
                else:
                    x = self.conv_group(x, conv, pad_mode, pad_override, None, act, act_param, label=lbl)
            elif hasattr(m, "conv_block"):      # ResnetBlock (models/networks.py:554-593)
                i += 1
                last_group = i >= n
                x = self.run_resblock(m, x, extra_add if last_group else None, "%s.%d" % (name, first_index + i - 1))
                if last_group:
                    extra_add = None
            elif isinstance(m, nn.Sequential):
                i += 1
                x = self.run_sequential(m, x, name="%s.%d" % (name, first_index + i - 1))
            elif isinstance(m, nn.Dropout):
                raise NotImplementedError("dropout is never enabled on the vid2vid path")
            else:
                raise NotImplementedError("module %r in %s" % (type(m), name))
            if collect is not None:
                collect.append(x)
        if extra_add is not None:
            x = self.add(x, extra_add)
        return x

    def run_resblock(self, blk, x, extra_add, name):
        mods = list(blk.conv_block)
        # [pad, conv, norm, act, pad, conv, norm]   (reflect) -- zero padding variant has no pad modules
        def take(j):
            pad_mode, pad_override = L.PAD_ZERO, None
            if isinstance(mods[j], nn.ReflectionPad2d):
                pad_mode, pad_override = L.PAD_REFLECT, int(mods[j].padding[0]); j += 1
            elif isinstance(mods[j], nn.ReplicationPad2d):
                raise NotImplementedError("replicate padding is not used by vid2vid")
            conv = mods[j]; norm = mods[j + 1]
            return pad_mode, pad_override, conv, norm, j + 2
        pm, po, conv1, norm1, j = take(0)
        act, act_param = self._act_code(mods[j]); j += 1
        h = self.conv_group(x, conv1, pm, po, norm1, act, act_param, label=name + ".c1")
        pm, po, conv2, norm2, j = take(j)
        return self.conv_group(h, conv2, pm, po, norm2, L.ACT_NONE, 0.0, add0=x, add1=extra_add, label=name + ".c2")

    # ---------------- other ops ----------------
    def _training(self):
        return self.plan is None and torch.is_grad_enabled()      # (dry-run engines build the autograd graph too)

    def add(self, a, b):
        if a.t.shape != b.t.shape:
            raise RuntimeError("add: shape mismatch %s vs %s" % (tuple(a.t.shape), tuple(b.t.shape)))
        if self._training() and (a.t.requires_grad or b.t.requires_grad):
            from . import autograd as AG
            return Act(AG.AddFn.apply(self, a.t, b.t), a.C)
        y = self.empty_act(a.N, a.H, a.W, a.C)
        check(lib.v2v_add_nhwc(_ptr(a.t), _ptr(b.t), _ptr(y.t), a.t.numel(), self.dtype, _stream()), "add")
        self.label("add_nhwc")
        return y

    def _fg_labels(self, fg_labels):
        """The foreground label ids on the device, built once per id list: torch.tensor(list, device=...) is a synchronous copy
        from pageable memory -- not permitted inside a stream capture (graphed.ChunkGraphs), and a host round trip per frame."""
        key = tuple(int(v) for v in fg_labels)
        cache = self.__dict__.setdefault("_fg_label_cache", {})
        t = cache.get(key)
        if t is None:
            t = cache[key] = torch.tensor(list(key), dtype=torch.int32, device=self.device)
        return t

    def fg_mask(self, x, base_ch, fg_labels):
        mask = self.empty_f32(x.N, 1, x.H, x.W)
        fg = self._fg_labels(fg_labels)
        self._keep(fg)
        check(lib.v2v_fg_mask_nhwc(_ptr(x.t), _ptr(mask), x.N * x.H * x.W, x.Cs, base_ch, _ptr(fg), fg.numel(),
                                   self.dtype, _stream()), "fg_mask")
        self.label("fg_mask_nhwc")
        return mask

    def last_planes(self, x_nchw, k):
        """The last k planes of every sample of planar fp32 (N, C, H, W) as a dense (N, k, H, W) tensor, by recordable copies
        (a view where it is dense already: N == 1, or k == C)."""
        v = x_nchw[:, -k:]
        if v.is_contiguous():
            return v
        out = self.empty_f32(x_nchw.shape[0], k, x_nchw.shape[2], x_nchw.shape[3])
        for n in range(x_nchw.shape[0]):
            self.memcpy(out[n], v[n], out[n].numel() * 4)
        return out

    def memcpy(self, dst, src, nbytes):
        check(lib.v2v_memcpy_d2d(_ptr(dst), _ptr(src), nbytes, _stream()), "memcpy_d2d")
        self.label("memcpy_d2d")

    def encode_labels_pooled(self, labels, inst, T, H, W, label_nc, fg_labels, want_mask, chunk_stride=False, source=None):
        """(lazy full-resolution Act, pooled Act, full-resolution mask): the encoded label maps one pyramid level down, straight
        from the maps (v2v_encode_labels_pooled).  The full-resolution Act carries only its LabelSource -- its tensor is allocated
        (shape / stride bookkeeping) but NEVER WRITTEN: legal only when every consumer reads the maps (gather-sum stems)."""
        per = label_nc + (1 if inst is not None else 0)
        bke = 64 if self.dtype == L.BF16 else 32
        cs = pad_channels(T * per, self.dtype)
        if chunk_stride:
            cs = (T * per + bke - 1) // bke * bke
        lazy = torch.empty((1, H, W, cs), dtype=self.tdtype, device=self.device)
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        pooled = torch.empty((1, OH, OW, cs), dtype=self.tdtype, device=self.device)
        self._keep(pooled)
        mask = self.empty_f32(1, 1, H, W) if want_mask else None
        fg = None
        if want_mask:
            fg = self._fg_labels(fg_labels)
            self._keep(fg)
        u8 = labels.dtype == torch.uint8
        if u8 and inst is not None and inst.dtype != torch.int32:
            raise TypeError("uint8 label maps go with int32 instance maps")
        if not u8 and (labels.dtype != torch.float32 or (inst is not None and inst.dtype != torch.float32)):
            raise TypeError("label / instance maps must be fp32-encoded integers, or uint8 + int32")
        codes = getattr(source, "codes", None) if source is not None else None
        if codes is not None and os.environ.get("V2V_POOLED_FROM_CODES", "1") != "0":
            # the frame plan has the 1-byte label | edge codes already (label_codes, for the gather-sum stems): nine independent byte
            # loads per frame instead of a chain of label / instance-map loads (394 -> see profiles/r05_*): same bits
            self._keep(codes)
            check(lib.v2v_encode_labels_pooled(_ptr(codes), _ptr(inst), _ptr(pooled), _ptr(mask), T, H, W, label_nc, cs, _ptr(fg),
                                               0 if fg is None else fg.numel(), self.dtype, 2, _stream()), "encode_labels_pooled (codes)")
        else:
            check(lib.v2v_encode_labels_pooled(_ptr(labels), _ptr(inst), _ptr(pooled), _ptr(mask), T, H, W, label_nc, cs, _ptr(fg),
                                               0 if fg is None else fg.numel(), self.dtype, int(u8), _stream()), "encode_labels_pooled")
        self.label("encode_labels_pooled")
        x0 = Act(lazy, T * per)
        x0.onehot = source if source is not None else LabelSource(labels, inst, T, label_nc)
        return x0, Act(pooled, T * per), mask

    def encode_labels(self, labels, inst, T, H, W, label_nc, fg_labels, want_mask, chunk_stride=False, source=None):
        """chunk_stride: pad the channel stride to a whole 128-byte K chunk (108 -> 128 channels) so that the
        narrow fine-scale 7x7 stems (cout <= 32) can run on the LDS-patch kernel (tile 60)."""
        per = label_nc + (1 if inst is not None else 0)
        N = labels.shape[0] if labels.dim() == 4 else 1      # multi-stream plans: maps (N, T, H, W), one launch per stream
        out = self.empty_act(N, H, W, T * per)
        if chunk_stride:
            bke = 64 if self.dtype == L.BF16 else 32
            cs = (T * per + bke - 1) // bke * bke
            wide = torch.empty((N, H, W, cs), dtype=self.tdtype, device=self.device)
            self._keep(wide)
            out = Act(wide, T * per)
        mask = self.empty_f32(N, 1, H, W) if want_mask else None
        fg = None
        if want_mask:
            fg = self._fg_labels(fg_labels)
            self._keep(fg)
        if labels.dtype == torch.uint8:              # uint8 label map + int32 instance map
            if inst is not None and inst.dtype != torch.int32:
                raise TypeError("uint8 label maps go with int32 instance maps")
            fn = lib.v2v_encode_labels_u8
        else:
            if labels.dtype != torch.float32 or (inst is not None and inst.dtype != torch.float32):
                raise TypeError("label / instance maps must be fp32-encoded integers, or uint8 + int32")
            fn = lib.v2v_encode_labels
        if N > 1:
            for n in range(N):
                check(fn(_ptr(labels[n]), _ptr(None if inst is None else inst[n]), _ptr(out.t[n]), _ptr(None if mask is None else mask[n]),
                         T, H, W, label_nc, out.Cs, _ptr(fg), 0 if fg is None else fg.numel(), self.dtype, _stream()),
                      "encode_labels")
                self.label("encode_labels")
            return out, mask          # no LabelSource: the stems run as convolutions on the encoding
        check(fn(_ptr(labels), _ptr(inst), _ptr(out.t), _ptr(mask), T, H, W, label_nc,
                 out.Cs, _ptr(fg), 0 if fg is None else fg.numel(), self.dtype, _stream()),
              "encode_labels")
        self.label("encode_labels")
        out.onehot = source if source is not None else LabelSource(labels, inst, T, label_nc)
        return out, mask

    def widen(self, x, stride):
        """Copy an activation into a zero-padded buffer with a larger channel stride (a whole 128-byte K chunk), so
        that a 7x7 head behind a 32-channel fine-scale tower can use the LDS-patch kernel."""
        wide = torch.zeros((x.N, x.H, x.W, stride), dtype=self.tdtype, device=self.device)
        self._keep(wide)
        check(lib.v2v_concat_channels_nhwc(_ptr(x.t), x.Cs, 0, _ptr(wide), stride, 0, x.C, x.N * x.H * x.W,
                                           self.dtype, _stream()), "widen")
        self.label("widen_nhwc")
        return Act(wide, x.C)

    def concat(self, a, b):
        """torch.cat([a, b], dim=1) on NHWC activations (inference / plan path; the pad channels of the result are zero)."""
        if (a.N, a.H, a.W) != (b.N, b.H, b.W):
            raise RuntimeError("concat: spatial shapes differ")
        if self._training() and (a.t.requires_grad or b.t.requires_grad):
            raise NotImplementedError("concat has no backward: the feature-encoding first-frame generators are inference-only")
        out = self.empty_act(a.N, a.H, a.W, a.C + b.C)
        if out.Cs != a.C + b.C:
            out.t.zero_()
        P = a.N * a.H * a.W
        check(lib.v2v_concat_channels_nhwc(_ptr(a.t), a.Cs, 0, _ptr(out.t), out.Cs, 0, a.C, P, self.dtype, _stream()), "concat")
        self.label("concat_nhwc")
        check(lib.v2v_concat_channels_nhwc(_ptr(b.t), b.Cs, 0, _ptr(out.t), out.Cs, a.C, b.C, P, self.dtype, _stream()), "concat")
        self.label("concat_nhwc")
        return out

    def pack(self, x_nchw):
        N, Cc, H, W = x_nchw.shape
        if self._training() and x_nchw.requires_grad:
            from . import autograd as AG
            return Act(AG.PackFn.apply(self, x_nchw, None, 1.0), Cc)
        out = self.empty_act(N, H, W, Cc)
        check(lib.v2v_pack_nchw_to_nhwc(_ptr(x_nchw), _ptr(out.t), N, Cc, H, W, out.Cs, self.dtype, _stream()), "pack")
        self.label("pack_nchw_to_nhwc")
        return out

    def unpack(self, x):
        if self._training() and x.t.requires_grad:
            from . import autograd as AG
            return AG.UnpackFn.apply(self, x.t, x.C)
        out = self.empty_f32(x.N, x.C, x.H, x.W)
        check(lib.v2v_unpack_nhwc_to_nchw(_ptr(x.t), _ptr(out), x.N, x.C, x.H, x.W, x.Cs, self.dtype, _stream()), "unpack")
        self.label("unpack_nhwc_to_nchw")
        return out

    def avgpool_nhwc(self, x):
        OH, OW = (x.H - 1) // 2 + 1, (x.W - 1) // 2 + 1
        if self._training() and x.t.requires_grad:
            from . import autograd as AG
            return Act(AG.AvgPoolFn.apply(self, x.t), x.C)
        out = self.empty_act(x.N, OH, OW, x.C)
        if out.Cs != x.Cs:                         # the kernel has ONE channel stride: keep the input's (chunk-padded labels)
            t = torch.empty((x.N, OH, OW, x.Cs), dtype=self.tdtype, device=self.device)
            self._keep(t)
            out = Act(t, x.C)
        check(lib.v2v_avgpool3s2_nhwc(_ptr(x.t), _ptr(out.t), x.N, x.H, x.W, x.Cs, self.dtype, _stream()), "avgpool_nhwc")
        self.label("avgpool3s2_nhwc")
        return out

    def maxpool2_nhwc(self, x):
        """MaxPool2d(2, 2) (VGG19 features inside Vgg19, models/networks.py:840-870)."""
        if self._training() and x.t.requires_grad:
            from . import autograd as AG
            return Act(AG.MaxPool2Fn.apply(self, x.t), x.C)
        t = torch.empty((x.N, x.H // 2, x.W // 2, x.Cs), dtype=self.tdtype, device=self.device)
        self._keep(t)
        check(lib.v2v_maxpool2_nhwc(_ptr(x.t), _ptr(t), x.N, x.H, x.W, x.Cs, self.dtype, _stream()), "maxpool2_nhwc")
        self.label("maxpool2_nhwc")
        return Act(t, x.C)

    def avgpool2_planar(self, x):
        """AvgPool2d(2, stride 2, count_include_pad=False) on planar fp32 [..., H, W] (VGGLoss.downsample)."""
        if self._training() and x.requires_grad:
            from . import autograd as AG
            return AG.AvgPool2PlanarFn.apply(self, x)
        x = x.contiguous().float()
        H, W = x.shape[-2], x.shape[-1]
        out = self.empty_f32(*x.shape[:-2], H // 2, W // 2)
        check(lib.v2v_avgpool2_planar(_ptr(x), _ptr(out), x.numel() // (H * W), H, W, _stream()), "avgpool2_planar")
        self.label("avgpool2_planar")
        return out

    def instance_mean(self, feat, inst):
        """Instance-wise average pooling (Encoder.forward, models/networks.py:621-632).  feat: planar fp32 (N, C, H, W);
        inst: (N, 1, H, W) fp32 holding integer ids.  Returns a tensor like feat."""
        feat = feat.contiguous().float()
        inst = inst.contiguous().float()
        N, Cc, H, W = feat.shape
        out = self.empty_f32(N, Cc, H, W)
        nbytes = lib.v2v_instance_mean_workspace(Cc, H * W)
        ws = self.scratch("instance_mean_ws", (nbytes + 3) // 4)
        for n in range(N):
            check(lib.v2v_instance_mean_planar(_ptr(feat[n]), _ptr(inst[n]), _ptr(out[n]), _ptr(ws), Cc, H * W, _stream()),
                  "instance_mean")
            self.label("instance_mean")
        return out

    def onehot_planar(self, labels, inst, H, W, label_nc):
        """Planar fp32 one-hot (+ edge plane) of one label frame: `real_A[0][0, -1]` (vid2vid_model_G.py:209)."""
        per = label_nc + (1 if inst is not None else 0)
        if labels.dim() == 3:         # multi-stream plans: one frame of every stream, a strided view (N, H, W) of (N, T, H, W) maps
            N = labels.shape[0]
            if labels.stride(1) != W or labels.stride(2) != 1 or (inst is not None and inst.stride() != labels.stride()):
                raise ValueError("onehot_planar: dense frames, the same sample stride for labels and instance maps")
            out = self.empty_f32(N, per, H, W)
            check(lib.v2v_onehot_planar_batch(_ptr(labels), _ptr(inst), int(labels.dtype == torch.uint8), _ptr(out), N,
                                              labels.stride(0), H, W, label_nc, _stream()), "onehot_planar_batch")
            self.label("onehot_planar")
            return out
        out = self.empty_f32(per, H, W)
        fn = lib.v2v_onehot_planar_u8 if labels.dtype == torch.uint8 else lib.v2v_onehot_planar
        check(fn(_ptr(labels), _ptr(inst), _ptr(out), H, W, label_nc, _stream()), "onehot_planar")
        self.label("onehot_planar")
        return out

    def avgpool_planar(self, x):
        """x: fp32 [..., H, W] contiguous -> [..., OH, OW]"""
        H, W = x.shape[-2], x.shape[-1]
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        planes = x.numel() // (H * W)
        out = self.empty_f32(*x.shape[:-2], OH, OW)
        check(lib.v2v_avgpool3s2_planar(_ptr(x), _ptr(out), planes, H, W, _stream()), "avgpool_planar")
        self.label("avgpool3s2_planar")
        return out

    def warp_blend(self, img_raw, flow, weight, prev, fg, mask, want_warp=False, roll=None, slot_mode=None, row_slot=None):
        """roll: the fp32 window (slots, C, H, W) of the last generated frames, oldest first -- the launch rolls it itself
        (v2v_warp_blend_roll; inference frame plans); (N, slots, C, H, W) for the N streams of a multi-stream plan
        (v2v_warp_blend_roll_batch).  `prev` must then be a buffer outside the window.
        slot_mode: int32 (N,) device tensor of per-stream modes (0 steady, 1 raw-only first frame, 2 idle), read by the launch
        when it runs (v2v_warp_blend_slots; slot plans); roll is then (N, slots, C, H, W) or None.
        row_slot: int32 (N,) device tensor, with slot_mode (0 or 1 only) and roll = the pool (S, slots, C, H, W): dense row n
        rolls slot row_slot[n] (v2v_warp_blend_pool; pool plans)."""
        N, Cc, H, W = img_raw.shape
        if self._training() and any(t is not None and t.requires_grad for t in (img_raw, flow, weight, prev, fg)):
            from . import autograd as AG
            final, raw_blend = AG.WarpBlendFn.apply(self, img_raw, flow, weight, prev, fg, mask)
            return (final, raw_blend), None
        gx, gy = self.grid(H, W)
        final = self.empty_f32(N, Cc, H, W)
        warp = self.empty_f32(N, Cc, H, W) if (want_warp and flow is not None) else None
        for t in (gx, gy):
            self._keep(t)
        words = [t for t in (slot_mode, row_slot) if t is not None]
        if row_slot is not None and (slot_mode is None or roll is None):
            raise ValueError("warp_blend: a pooled blend rolls an fp32 pool (S, slots, C, H, W) under int32 slot_mode, row_slot (N,)")
        if any(t.dtype != torch.int32 or tuple(t.shape) != (N,) or not t.is_contiguous() for t in words):
            raise ValueError("warp_blend: slot_mode and row_slot are int32 (N,)")
        if roll is not None:
            lead = tuple(roll.shape[:-4])        # () one sample's window, (N,) one per stream, (S,) the pool row_slot indexes
            if (roll.dim() < 4 or tuple(roll.shape[-3:]) != (Cc, H, W) or roll.dtype != torch.float32 or not roll.is_contiguous()
                    or not (len(lead) == 1 if row_slot is not None else lead == (N,) or (lead == () and N == 1 and not words))):
                raise ValueError("warp_blend: the rolled window is fp32 (slots, C, H, W) of one sample, (N, slots, C, H, W) of N "
                                 "streams, or with row_slot the pool (S, slots, C, H, W)")
        for t in words:
            self._keep(t)
        # the entry point, and what it takes between gy and C
        win = (_ptr(roll), 0 if roll is None else roll.shape[-4])
        if row_slot is not None:
            entry, extra = "warp_blend_pool", win + (_ptr(slot_mode), _ptr(row_slot), N, roll.shape[0])
        elif slot_mode is not None:
            entry, extra = "warp_blend_slots", win + (_ptr(slot_mode), N)
        elif roll is None:
            entry, extra = "warp_blend", (N,)
        else:
            entry, extra = ("warp_blend_roll", win) if roll.dim() == 4 else ("warp_blend_roll_batch", win + (N,))
        check(getattr(lib, "v2v_" + entry)(_ptr(img_raw), _ptr(flow), _ptr(weight), _ptr(prev), _ptr(fg), _ptr(mask), _ptr(final),
                                           _ptr(warp), _ptr(gx), _ptr(gy), *extra, Cc, H, W, int(self.align_corners), _stream()), entry)
        self.label("warp_blend")
        return final, warp

    def window_roll(self, window, frame, slot_mode):
        """window (N, slots, C, H, W) <- frame (N, C, H, W) for the streams whose slot_mode is 0 or 1; an idle stream's window
        is not touched (v2v_window_roll_slots: one launch instead of N * slots device copies)."""
        N, slots, Cc, H, W = window.shape
        if (tuple(frame.shape) != (N, Cc, H, W) or tuple(slot_mode.shape) != (N,) or slot_mode.dtype != torch.int32
                or window.dtype != torch.float32 or frame.dtype != torch.float32
                or not (window.is_contiguous() and frame.is_contiguous() and slot_mode.is_contiguous())):
            raise ValueError("window_roll: fp32 window (N, slots, C, H, W), fp32 frame (N, C, H, W), int32 slot_mode (N,)")
        self._keep(slot_mode)
        check(lib.v2v_window_roll_slots(_ptr(window), _ptr(frame), _ptr(slot_mode), N, slots, Cc, H, W, _stream()),
              "window_roll_slots")
        self.label("window_roll")

    def _window_pool_args(self, dense, pool, row_slot, what):
        K, S = dense.shape[0], pool.shape[0]
        if (dense.dim() != 5 or pool.dim() != 5 or tuple(dense.shape[1:]) != tuple(pool.shape[1:]) or tuple(row_slot.shape) != (K,)
                or row_slot.dtype != torch.int32 or dense.dtype != torch.float32 or pool.dtype != torch.float32
                or not (dense.is_contiguous() and pool.is_contiguous() and row_slot.is_contiguous())):
            raise ValueError("%s: fp32 dense (K, slots, C, H, W), fp32 pool (S, slots, C, H, W), int32 row_slot (K,)" % what)
        self._keep(row_slot)
        return (_ptr(row_slot), K, S) + tuple(dense.shape[1:]) + (_stream(),)

    def window_gather(self, dense, pool, row_slot):
        """dense (K, slots, C, H, W) <- pool[row_slot[k]] of the pool (S, slots, C, H, W), one launch (v2v_window_gather_pool)."""
        check(lib.v2v_window_gather_pool(_ptr(dense), _ptr(pool), *self._window_pool_args(dense, pool, row_slot, "window_gather")),
              "window_gather_pool")
        self.label("window_gather")

    def window_scatter(self, pool, dense, row_slot):
        """pool[row_slot[k]] <- dense[k], the inverse of window_gather (v2v_window_scatter_pool); other slots are not touched."""
        check(lib.v2v_window_scatter_pool(_ptr(pool), _ptr(dense), *self._window_pool_args(dense, pool, row_slot, "window_scatter")),
              "window_scatter_pool")
        self.label("window_scatter")

    def frames_u8(self, frames, mode=None, row_slot=None, S=None, normalize=True):
        """uint8 images (S, H, W, C) of the fp32 planar rows `frames` (K, C, H, W) in one launch (v2v_frames_u8): image
        s is tensor2im of the row k with row_slot[k] == s (row s without row_slot; S = K then) whose mode[k] is 0 or 1, and all
        zero bytes where there is none.  mode / row_slot: int32 (K,) device tensors read when the launch runs, or None.  The
        launch writes every byte of the image buffer it returns."""
        K, Cc, H, W = frames.shape
        S = K if S is None else int(S)
        if frames.dtype != torch.float32 or not frames.is_contiguous():
            raise ValueError("frames_u8: contiguous fp32 frames (K, C, H, W)")
        for t in (mode, row_slot):
            if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (K,) or not t.is_contiguous()):
                raise ValueError("frames_u8: mode and row_slot are int32 (K,)")
            if t is not None:
                self._keep(t)
        out = torch.empty((S, H, W, Cc), dtype=torch.uint8, device=self.device)
        self._keep(out)
        check(lib.v2v_frames_u8(_ptr(frames), _ptr(out), _ptr(mode), _ptr(row_slot), K, S, Cc, H, W, int(bool(normalize)),
                                _stream()), "frames_u8")
        self.label("frames_u8")
        return out

    def label_image(self, labels, inst, label_nc, slot_mode=None, row_slot=None, S=None):
        """uint8 pictures (S, H, W, 3) of the newest frame of the label maps `labels` (K, T, H, W) -- uint8 with int32 `inst`, or
        fp32-encoded integers with fp32 `inst`; inst may be None -- in one launch (v2v_label_image): image s is, bit
        for bit, visual.tensor2label(onehot_planar(labels[k, T - 1], inst[k, T - 1]), label_nc) of the row k with row_slot[k] == s
        (row s without row_slot; S = K then) whose slot_mode[k] is 0 or 1, and all zero bytes where there is none.  slot_mode /
        row_slot: int32 (K,) device tensors read when the launch runs, or None.  The launch writes every byte of the buffer."""
        if labels.dim() != 4 or not labels.is_contiguous() or labels.dtype not in (torch.uint8, torch.float32):
            raise ValueError("label_image: contiguous uint8 or fp32 label maps (K, T, H, W)")
        K, T, H, W = labels.shape
        u8 = labels.dtype == torch.uint8
        if inst is not None and (inst.dtype != (torch.int32 if u8 else torch.float32) or inst.shape != labels.shape
                                 or not inst.is_contiguous()):
            raise ValueError("label_image: the instance maps are int32 beside uint8 labels, fp32 beside fp32 ones, of their shape")
        if not 1 <= label_nc <= 255:
            raise ValueError("label_image: label_nc within 1..255, got %d" % label_nc)
        S = K if S is None else int(S)
        for t in (slot_mode, row_slot):
            if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (K,) or not t.is_contiguous()):
                raise ValueError("label_image: slot_mode and row_slot are int32 (K,)")
            if t is not None:
                self._keep(t)
        cmap = self._label_cmaps.get(label_nc)
        if cmap is None:
            from .visual import labelcolormap
            cmap = self._label_cmaps[label_nc] = torch.from_numpy(labelcolormap(label_nc)[:label_nc].copy()).to(self.device)
        out = torch.empty((S, H, W, 3), dtype=torch.uint8, device=self.device)
        for t in (labels, inst, cmap, out):
            if t is not None:
                self._keep(t)
        check(lib.v2v_label_image(_ptr(labels), _ptr(inst), int(u8), _ptr(cmap), label_nc, _ptr(out), _ptr(slot_mode), _ptr(row_slot),
                                  K, S, T, H, W, _stream()), "label_image")
        self.label("label_image")
        return out

    def resample_flow(self, img, flow):
        N, Cc, H, W = img.shape
        if self._training() and (img.requires_grad or flow.requires_grad):
            from . import autograd as AG
            return AG.ResampleFn.apply(self, img, flow)
        gx, gy = self.grid(H, W)
        out = self.empty_f32(N, Cc, H, W)
        check(lib.v2v_resample_flow(_ptr(img), _ptr(flow), _ptr(out), _ptr(gx), _ptr(gy), N, Cc, H, W,
                                    int(self.align_corners), _stream()), "resample_flow")
        self.label("resample_flow")
        return out
