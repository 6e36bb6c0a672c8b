"""On-GPU counterparts of the reference's util/util.py tensor -> image helpers.

The reference's test.py (:43-54) converts every generated frame on the host: a D2H copy of the fp32 planes (36 x H x W floats for
the label map alone), then numpy (`util.tensor2label`, `util.tensor2im`), then PIL.  Here the conversion is a HIP kernel on the
device and only the uint8 HWC image crosses PCIe; `AsyncImageWriter` encodes / writes files on a worker thread so the save path
does not stall a generator that runs at hundreds of frames per second.

    tensor2im(t, normalize=True)  -> uint8 device tensor (H, W, C) or (H, W) for one plane      (util/util.py:48-71)
    tensor2im_batch(t, normalize) -> uint8 device tensor (B, H, W, C) of (B, C, H, W), one launch for all samples
    tensor2label(t, n_label)      -> uint8 device tensor (H, W, 3)                              (util/util.py:73-87)
    tensor2flow(t)                -> uint8 device tensor (H, W, 3), HSV-coded flow picture      (util/util.py:89-107)
    to_numpy(img)                 -> what the reference's function returns (numpy uint8)
"""
import ctypes as C
import operator
import queue
import threading

import numpy as np
import torch

from .lib import lib, check

# Cityscapes palettes of util/util.py:156-168 (label ids -> RGB; the public Cityscapes colour coding)
_CITY35 = [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (111, 74, 0), (81, 0, 81), (128, 64, 128), (244, 35, 232),
           (250, 170, 160), (230, 150, 140), (70, 70, 70), (102, 102, 156), (190, 153, 153), (180, 165, 180), (150, 100, 100),
           (150, 120, 90), (153, 153, 153), (153, 153, 153), (250, 170, 30), (220, 220, 0), (107, 142, 35), (152, 251, 152),
           (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70), (0, 60, 100), (0, 0, 90), (0, 0, 110),
           (0, 80, 100), (0, 0, 230), (119, 11, 32), (0, 0, 142)]
_CITY20 = [(128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153), (250, 170, 30),
           (220, 220, 0), (107, 142, 35), (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70),
           (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32), (0, 0, 0)]


def labelcolormap(n):
    """util/util.py:156-181: the two Cityscapes tables, otherwise the bit-interleaved PASCAL-style map."""
    if n == 35:
        return np.array(_CITY35, dtype=np.uint8)
    if n == 20:
        return np.array(_CITY20, dtype=np.uint8)
    cmap = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        r = g = b = 0
        idx = i
        for j in range(7):
            r ^= (idx & 1) << (7 - j)
            g ^= ((idx >> 1) & 1) << (7 - j)
            b ^= ((idx >> 2) & 1) << (7 - j)
            idx >>= 3
        cmap[i] = (r, g, b)
    return cmap


_CMAPS = {}


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _planes(t):
    """The reference's leading-dim rules (util/util.py:57-60): 5-D -> [0, -1], 4-D -> [0]."""
    if t.dim() == 5:
        t = t[0, -1]
    if t.dim() == 4:
        t = t[0]
    return t.detach().float().contiguous()


def tensor2im(image_tensor, normalize=True):
    if isinstance(image_tensor, list):
        return [tensor2im(t, normalize) for t in image_tensor]
    x = _planes(image_tensor)[:3].contiguous()
    Cc, H, W = x.shape
    out = torch.empty((H, W, Cc), dtype=torch.uint8, device=x.device)
    check(lib.v2v_tensor2im(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), Cc, H, W, int(bool(normalize)), _stream(x)),
          "tensor2im")
    return out[:, :, 0] if Cc == 1 else out


def tensor2im_batch(image_tensor, normalize=True):
    """tensor2im of every sample of (B, C, H, W), C <= 4, in one launch (v2v_frames_u8): uint8 (B, H, W, C), sample b bit for bit
    tensor2im(image_tensor[b]).  (Frame plans of a model with opt.frames_u8 record the same launch as their last op.)"""
    if image_tensor.dim() != 4:
        raise ValueError("tensor2im_batch expects (B, C, H, W), got %s" % (tuple(image_tensor.shape),))
    x = image_tensor.detach().float().contiguous()
    B, Cc, H, W = x.shape
    out = torch.empty((B, H, W, Cc), dtype=torch.uint8, device=x.device)
    check(lib.v2v_frames_u8(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), None, None, B, B, Cc, H, W, int(bool(normalize)),
                            _stream(x)), "frames_u8")
    return out


def input_lut(in_ch, densepose_part_channel=None):
    """The value table of uint8 image inputs (opt.inputs_u8): fp32 (in_ch, 256), row c the reference loader's
    transform of every byte of channel c, by the loader's own fp32 operations in its order -- ToTensor (byte / 255) then
    Normalize(0.5, 0.5) ((v - 0.5) / 0.5; data/base_dataset.py:148-157), and for `densepose_part_channel` (2 in the pose recipes)
    the part-index rescale behind them, ((v * 0.5 + 0.5) * 255 / 24 - 0.5) / 0.5 (data/pose_dataset.py:44).  Nearest resize and
    crop commute with a per-byte function, so decoding a byte through this table equals loading it through the reference."""
    if in_ch < 1:
        raise ValueError("input_lut: in_ch >= 1")
    if densepose_part_channel is not None and not 0 <= densepose_part_channel < in_ch:
        raise ValueError("input_lut: part channel %r of %d channels" % (densepose_part_channel, in_ch))
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    v = v.sub(torch.tensor(0.5)).div(torch.tensor(0.5))
    lut = v.repeat(in_ch, 1)
    if densepose_part_channel is not None:
        lut[densepose_part_channel] = ((v * 0.5 + 0.5) * 255 / 24 - 0.5) / 0.5
    return lut.contiguous()


def decode_inputs(input_u8, lut):
    """fp32 planes (..., C, H, W) of uint8 HWC frames (..., H, W, C) through the table `lut` (C, 256): a torch gather, for the
    paths off the frame plan (first frames, references in tests)."""
    C_ = input_u8.shape[-1]
    lut = lut.to(input_u8.device)
    planes = input_u8.movedim(-1, -3).long()                                 # (..., C, H, W)
    idx = planes + (torch.arange(C_, device=input_u8.device) * 256).view(C_, 1, 1)
    return lut.reshape(-1)[idx]


GEOMETRY_MAX_SIZE = 16384      # of a source frame and of new_size: keeps (2 xr + 1) Ws inside int32 (include/v2v_hip.h)


def _int_pair(value, what):
    try:
        a, b = value
        return operator.index(a), operator.index(b)
    except (TypeError, ValueError):
        raise ValueError("input geometry: %s is a pair of integers, got %r" % (what, value)) from None


def geometry_words(geometry):
    """(new_w, new_h, x1, y1, flip, H, W) of one geometry: the reference's get_img_params dict (data/base_dataset.py:85-128) --
    new_size=(new_w, new_h); crop_size=(cw, ch), (0, 0) or missing for no crop stage; crop_pos=(x1, y1); flip=bool -- as
    get_transform applies it with method=Image.NEAREST (:130-175): resize to new_size, then __crop (only if the resized frame
    is wider or higher than crop_size, with the box clipped to the frame), then FLIP_LEFT_RIGHT.  x1, y1 are 0 where nothing
    is cropped (crop_pos is then not looked at, as in the reference); (H, W) is the size of the result.  ValueError for
    anything else."""
    if not isinstance(geometry, dict):
        raise ValueError("input geometry: a dict with the keys of get_img_params (new_size, crop_size, crop_pos, flip), got %r"
                         % type(geometry).__name__)
    unknown = set(geometry) - {"new_size", "crop_size", "crop_pos", "flip"}
    if unknown or "new_size" not in geometry:
        raise ValueError("input geometry: keys new_size (required), crop_size, crop_pos, flip; got %s" % sorted(geometry))
    new_w, new_h = _int_pair(geometry["new_size"], "new_size")
    if not (1 <= new_w <= GEOMETRY_MAX_SIZE and 1 <= new_h <= GEOMETRY_MAX_SIZE):
        raise ValueError("input geometry: new_size within 1..%d, got %r" % (GEOMETRY_MAX_SIZE, (new_w, new_h)))
    flip = geometry.get("flip", False)
    if not isinstance(flip, (bool, np.bool_)):
        raise ValueError("input geometry: flip is a bool, got %r" % (flip,))
    cw, ch = _int_pair(geometry.get("crop_size", (0, 0)), "crop_size")
    if cw < 0 or ch < 0:
        raise ValueError("input geometry: crop_size is not negative, got %r" % ((cw, ch),))
    x1 = y1 = 0
    W, H = new_w, new_h
    if (cw, ch) != (0, 0):                                             # a crop stage: its corner is checked even where
        px, py = _int_pair(geometry.get("crop_pos", (0, 0)), "crop_pos")    # __crop then keeps the whole frame
        if not (0 <= px < new_w and 0 <= py < new_h):
            raise ValueError("input geometry: crop_pos %r is outside the resized %dx%d frame" % ((px, py), new_w, new_h))
        if new_w > cw or new_h > ch:                                   # __crop: if (ow > tw or oh > th)
            x1, y1 = px, py
            W, H = min(new_w, x1 + cw) - x1, min(new_h, y1 + ch) - y1
            if W < 1 or H < 1:
                raise ValueError("input geometry: crop_size %r leaves an empty frame" % ((cw, ch),))
    return new_w, new_h, x1, y1, int(bool(flip)), H, W


def geometry_size(geometry):
    """(H, W) of the frame that a geometry (geometry_words) yields: the size of the model's inputs under opt.input_geometry."""
    return geometry_words(geometry)[5:]


def gather_entries(t_in, tG, rows, new, per_stream):
    """The entry table of one inference call under opt.input_geometry: input_A is (B, t_in, ...) viewed as B t_in
    source frames, the uint8 windows (B or S, tG, ...) viewed as frames.  A stream of `new` (started or restarted) sends all its
    t_in == tG frames to its window's slots; every other stream of `rows` (the active ones) sends its newest frame to slot
    tG - 1; streams outside `rows` get no entry.  [src_frame, dst_frame, geom, 0] per entry, geom = the stream with a geometry
    per stream, else 0."""
    entries = []
    for b in rows:
        g = b if per_stream else 0
        if b in new:
            if t_in != tG:
                raise ValueError("a started stream brings its whole window (t = %d), got t = %d" % (tG, t_in))
            entries += [[b * t_in + t, b * tG + t, g, 0] for t in range(tG)]
        else:
            entries.append([b * t_in + t_in - 1, b * tG + tG - 1, g, 0])
    return entries


def resample_u8(src, geometry, out=None):
    """uint8 frames (F, Hs, Ws, C) -> (F, H, W, C) under one geometry (geometry_words), by v2v_gather_frames_u8 on its own: the
    reference loader's img.resize(new_size, Image.NEAREST), __crop and flip of every frame, byte for byte.  The bytes may be
    anything -- image channels or label / instance ids (the loaders resize label maps with NEAREST too).  out: a contiguous
    uint8 device tensor (F, H, W, C) to write into."""
    if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or src.dim() != 4:
        raise ValueError("resample_u8: uint8 frames (F, Hs, Ws, C)")
    words = geometry_words(geometry)
    F, Hs, Ws, Cc = src.shape
    H, W = words[5:]
    if not (1 <= Hs <= GEOMETRY_MAX_SIZE and 1 <= Ws <= GEOMETRY_MAX_SIZE and 1 <= Cc <= 32 and F >= 1):
        raise ValueError("resample_u8: frames of 1..%d rows and columns and 1..32 channels, got %s" % (GEOMETRY_MAX_SIZE, tuple(src.shape)))
    if not src.is_cuda and not lib.v2v_get_dry_run():
        raise ValueError("resample_u8: the frames are in device memory")
    src = src.contiguous()
    if out is None:
        out = torch.empty((F, H, W, Cc), dtype=torch.uint8, device=src.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (F, H, W, Cc)
          or not out.is_contiguous() or out.device != src.device):
        raise ValueError("resample_u8: out is contiguous uint8 %s on the frames' device" % ((F, H, W, Cc),))
    # entries [F][4] then the geometry [8], one int32 buffer (both tables 16-byte aligned)
    table = torch.tensor([w for f in range(F) for w in (f, f, 0, 0)] + list(words[:5]) + [0, 0, 0], dtype=torch.int32).to(src.device)
    check(lib.v2v_gather_frames_u8(C.c_void_p(src.data_ptr()), F, Hs, Ws, C.c_void_p(out.data_ptr()), F, H, W, Cc,
                                   C.c_void_p(table.data_ptr()), F, C.c_void_p(table.data_ptr() + 16 * F), 1, _stream(src)),
          "gather_frames_u8")
    return out


def tensor2label(output, n_label):
    x = _planes(output)
    Cc, H, W = x.shape
    key = (n_label, str(x.device))
    if key not in _CMAPS:
        _CMAPS[key] = torch.from_numpy(labelcolormap(n_label)[:n_label].copy()).to(x.device)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
    check(lib.v2v_tensor2label(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(_CMAPS[key].data_ptr()),
                               n_label, Cc, H, W, _stream(x)), "tensor2label")
    return out


def tensor2flow(output):
    """util/util.py:89-107 (used by save_all_tensors :38-41 for `flow_ref` and `flow`): direction -> hue, magnitude (min-max
    normalised over the image) -> value.  The reference computes it with OpenCV on the host after a D2H copy of the flow."""
    x = _planes(output)
    if x.shape[0] != 2:
        raise ValueError("tensor2flow expects 2 flow planes, got %d" % x.shape[0])
    _, H, W = x.shape
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
    ws = torch.empty(2, dtype=torch.int32, device=x.device)
    check(lib.v2v_tensor2flow(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), H, W, _stream(x)),
          "tensor2flow")
    return out


def to_numpy(img):
    return img.cpu().numpy()


class AsyncImageWriter:
    """Saves uint8 HWC device images without stalling the caller: the D2H copy goes to a pinned staging buffer on a side
    stream, file encoding / writing (PIL, as util.save_image :127-129) happens on a worker thread.
        w = AsyncImageWriter(); w.save(tensor2im(fake_B), "out/frame0001.jpg"); ...; w.close()"""

    def __init__(self, depth=8):
        self.q = queue.Queue(maxsize=depth)
        self.stream = torch.cuda.Stream() if torch.cuda.is_available() else None
        self.errors = []
        self.worker = threading.Thread(target=self._run, daemon=True)
        self.worker.start()

    def _run(self):
        from PIL import Image
        while True:
            item = self.q.get()
            if item is None:
                return
            host, event, path = item
            try:
                if event is not None:
                    event.synchronize()
                Image.fromarray(host.numpy()).save(path)
            except Exception as ex:          # surfaced by close()
                self.errors.append((path, ex))

    def save(self, img, path):
        if img.is_cuda:
            host = torch.empty(img.shape, dtype=torch.uint8, pin_memory=True)
            self.stream.wait_stream(torch.cuda.current_stream(img.device))
            with torch.cuda.stream(self.stream):
                host.copy_(img, non_blocking=True)
                event = torch.cuda.Event()
                event.record(self.stream)
            img.record_stream(self.stream)
        else:
            host, event = img.clone(), None
        self.q.put((host, event, path))

    def close(self):
        self.q.put(None)
        self.worker.join()
        if self.errors:
            raise RuntimeError("image writer failed: %s" % self.errors[:3])
