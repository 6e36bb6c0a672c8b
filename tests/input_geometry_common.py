"""opt.input_geometry: an independent numpy restatement of the loaders' nearest resize, crop and flip as index maps,
shared by the CPU tests (which hold it against Pillow) and the GPU tests (which hold the kernel and the model against it).

    img.resize((new_w, new_h), Image.NEAREST)   then   __crop (only if ow > tw or oh > th; box clipped to the frame)
    then   FLIP_LEFT_RIGHT if flip                                                  (data/base_dataset.py:130-175)

Pillow's nearest filter takes, for destination column xr of new_w, source column floor((xr + 0.5) * Ws / new_w), which in integers is
((2 xr + 1) Ws) // (2 new_w); rows likewise."""
import numpy as np


def box(geom):
    """(x1, y1, W, H) of the frame a geometry keeps of the resized new_w x new_h one."""
    new_w, new_h = geom["new_size"]
    tw, th = geom.get("crop_size", (0, 0))
    x1 = y1 = 0
    W, H = new_w, new_h
    if (tw, th) != (0, 0) and (new_w > tw or new_h > th):
        x1, y1 = geom.get("crop_pos", (0, 0))
        W, H = min(new_w, x1 + tw) - x1, min(new_h, y1 + th) - y1
    return int(x1), int(y1), int(W), int(H)


def index_maps(Hs, Ws, geom):
    """(src_y[H], src_x[W]) int64: destination pixel (y, x) is source pixel (src_y[y], src_x[x])."""
    new_w, new_h = geom["new_size"]
    x1, y1, W, H = box(geom)
    x = np.arange(W, dtype=np.int64)
    if geom.get("flip", False):
        x = W - 1 - x
    src_x = ((2 * (x + x1) + 1) * Ws) // (2 * new_w)
    src_y = ((2 * (np.arange(H, dtype=np.int64) + y1) + 1) * Hs) // (2 * new_h)
    assert src_x.min() >= 0 and src_x.max() < Ws and src_y.min() >= 0 and src_y.max() < Hs
    return src_y, src_x


def gather(src, geom):
    """Frames (..., Hs, Ws, C), a numpy array or a torch tensor, resized / cropped / flipped: (..., H, W, C) of the same kind."""
    Hs, Ws = src.shape[-3:-1]
    src_y, src_x = index_maps(Hs, Ws, geom)
    if isinstance(src, np.ndarray):
        return np.ascontiguousarray(src[..., src_y[:, None], src_x[None, :], :])
    import torch
    sy, sx = torch.from_numpy(src_y).to(src.device), torch.from_numpy(src_x).to(src.device)
    return src[..., sy[:, None], sx[None, :], :].contiguous()
