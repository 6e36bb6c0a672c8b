"""The input picture of a label frame (opt.real_A_u8), restated in torch without any project code but the
palette: label map + instance map -> one-hot planes and edge plane as the reference's encode_input / get_edges build them
(models/vid2vid_model_G.py:86-112, models/base_model.py:146-152) -> util.tensor2label (util/util.py:73-87: the first maximum
over the planes, coloured through labelcolormap, no colour for an index the palette does not have).  Shared by the CPU and the
GPU tests of the option."""
import torch


def edges(inst):
    """get_edges on one (H, W) map: a pixel is an edge where its id differs from a 4-neighbour inside the image."""
    e = torch.zeros(inst.shape, dtype=torch.bool)
    dx = inst[:, 1:] != inst[:, :-1]
    dy = inst[1:, :] != inst[:-1, :]
    e[:, 1:] |= dx
    e[:, :-1] |= dx
    e[1:, :] |= dy
    e[:-1, :] |= dy
    return e


def planes_of(labels, inst, label_nc):
    """fp32 (label_nc [+ 1], H, W): plane c is 1 where the label is c (a label the one-hot has no plane for sets none), the last
    plane the instance edges.  Labels stored as floats are integers, read by truncation."""
    lab = labels.cpu().to(torch.int64)
    planes = torch.stack([(lab == c) for c in range(label_nc)]).float()
    if inst is not None:
        planes = torch.cat([planes, edges(inst.cpu())[None].float()])
    return planes


def picture_of_planes(planes, label_nc, cmap):
    """tensor2label: uint8 (H, W, 3).  More than one plane: the index of the first maximum; one plane: its stored value."""
    C, H, W = planes.shape
    if C > 1:
        top = planes.max(0).values
        order = torch.arange(C).view(C, 1, 1).expand(C, H, W)
        idx = torch.where(planes == top, order, torch.full_like(order, C)).min(0).values
    else:
        idx = planes[0].to(torch.int64)
    out = torch.zeros(H, W, 3, dtype=torch.uint8)
    cmap = torch.as_tensor(cmap)
    for c in range(label_nc):
        out[idx == c] = cmap[c]
    return out


def picture(labels, inst, label_nc):
    """The picture of one (H, W) label map (any dtype holding integers) and its instance map (or None)."""
    from vid2vid_amd.visual import labelcolormap
    return picture_of_planes(planes_of(labels, inst, label_nc), label_nc, labelcolormap(label_nc))


def planted_maps(N, T, H, W, label_nc, seed, all_values=True):
    """uint8 labels and int32 instance ids (N, T, H, W).  Frames 0..T-2 hold other labels and ids than the newest one (a wrong
    frame index shows).  The newest frame: random labels inside the palette; where the map is large enough every byte value
    0..255 is planted; labels outside the palette sit on instance edges and inside flat instance regions, in the image's
    corners and on its border; the instance map is blocks of 3x5 pixels, so edges touch every border."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, label_nc, (N, T, H, W), generator=g, dtype=torch.int64)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    blocks = (yy // 3) * 1000 + xx // 5
    inst = torch.stack([torch.stack([blocks * (n + 2) + 7 * t for t in range(T)]) for n in range(N)])
    for n in range(N):
        new = lab[n, T - 1].view(-1)
        fixed = {}
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, 0), (0, W // 2)):
            fixed[y * W + x] = 255 - (y + x) % 3
        # one flat instance region around an out-of-range label, one isolated instance pixel under another
        if H >= 5 and W >= 7:
            inst[n, T - 1, 1:4, 1:6] = 5
            fixed[2 * W + 3] = label_nc
            inst[n, T - 1, H - 2, W - 2] = 99999
            fixed[(H - 2) * W + W - 2] = 200
        free = [p for p in torch.randperm(H * W, generator=g).tolist() if p not in fixed]
        if all_values and len(free) >= 512:
            new[free[:256]] = torch.arange(256)
        else:
            pos = free[:max(1, len(free) // 3)]
            new[pos] = torch.randint(label_nc, 256, (len(pos),), generator=g)
        for p, v in fixed.items():
            new[p] = v
    return lab.to(torch.uint8), inst.to(torch.int32)
