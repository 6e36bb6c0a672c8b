"""Vid2VidModelG on the MI355X backend.

API-compatible with the reference's models/vid2vid_model_G.py: `initialize(opt)`,
`inference(input_A, input_B, inst_A) -> (fake_B, real_A_last)` with the rolling
`self.fake_B_prev` state reset by assigning None (test.py:34-35), `forward(...)` for training,
`compute_mask`, `compute_fake_B_prev`, `save`.

Inference is plan based: the first call at a given resolution lowers the whole per-frame
computation (input encoding -> label pyramid -> coarse-to-fine generators -> warp/blend ->
rolling window update; reference :198-229) to a recorded launch sequence over preallocated
buffers, instantiates it as a hipGraph, and every later frame is: refresh the input buffers,
one graph launch.  The reference issues ~240 framework ops per frame from Python instead.
"""
import os

import torch

from .. import lib as L
from .. import networks
from ..engine import Act, Plan
from ..optim import FusedAdam
from .base_model import BaseModel


def nearest_face_features(feat_map, inst, features, feat_num):
    """Second half of get_face_features (reference models/vid2vid_model_G.py:296-320): pick the training image whose
    per-part encoder features are nearest to this image's (squared distance summed over the facial parts present and the
    feat_num channels; dists_min, base_model.py:136-144) and paint ITS features over the parts.
    feat_map: (N, >=feat_num, H, W) instance-wise constant encoder output; inst: (N, 1, H, W) part ids in 0..6;
    features: {part id: array (num_images_of_part, feat_num + 1)} (checkpoints/edge2face_single/features.npy).
    Parts absent from `inst` contribute nothing (the reference leaves their rows of the two scratch tensors uninitialised)."""
    import numpy as np
    inst_l = inst.long()
    labels = [int(l) for l in torch.unique(inst_l)]
    num_images = features[6].shape[0]
    ori = torch.zeros(7, feat_num, 1)
    ref = torch.zeros(7, feat_num, num_images)
    for label in labels:
        idx = (inst_l == label).nonzero()
        b, _, y, x = [int(v) for v in idx[0]]
        ori[label, :, 0] = feat_map[b, :feat_num, y, x].detach().float().cpu()
        ref[label] = torch.from_numpy(np.ascontiguousarray(features[label][:num_images, :feat_num].T)).float()
    dists = ((ori - ref) ** 2).sum(0).sum(0)
    cluster = int(torch.argmin(dists))
    out = torch.zeros(inst.size(0), feat_num, inst.size(2), inst.size(3), dtype=torch.float32, device=inst.device)
    for label in labels:
        feat = features[label][:, :-1]
        row = torch.as_tensor(np.asarray(feat[min(cluster, feat.shape[0] - 1), :feat_num], dtype=np.float32), device=inst.device)
        mask = (inst_l[:, 0] == label)                                   # (N, H, W)
        out.permute(0, 2, 3, 1)[mask] = row
    return out


class _StreamPool:
    """The windows of the S stream slots of a compacting model (opt.compact_streams): fake_B_prev per scale,
    (S, tG-1, 3, h, w), owned by the model -- every pool plan of this resolution, whatever its row count K, reaches them through
    its row_slot indices, so changing K between calls copies nothing.  `idle`: the slots whose rows of the tensors the last call
    returned are zero.  `inputs` (opt.inputs_u8_slots): the uint8 input windows of the slots, (S, tG, H, W, in_ch) per
    in_ch, allocated at first use and reached through row_slot like the generated windows."""

    def __init__(self, S, tG, nc, H, W, n_scales, device):
        self.S, self.H, self.W = S, H, W
        self.tG, self.device = tG, device
        self.windows = [torch.zeros(S, tG - 1, nc, H >> si, W >> si, dtype=torch.float32, device=device) for si in range(n_scales)]
        self.inputs = {}
        self.idle = []

    def input_windows(self, in_ch):
        win = self.inputs.get(in_ch)
        if win is None:
            win = self.inputs[in_ch] = torch.zeros(self.S, self.tG, self.H, self.W, in_ch, dtype=torch.uint8, device=self.device)
        return win


class _FramePlan:
    """Buffers + launch sequence generating one frame at every spatial scale, for B independent sequences (streams) per
    replay.  B == 1: the buffers have no stream dimension, exactly the single-sequence plan.  B > 1: every static
    buffer and output gets a leading B, and every norm group is lowered with per-sample statistics (Engine.per_stream), so
    stream b computes what a batch-1 plan computes on sequence b alone.
    slots (B > 1): the plan owns `slot_mode`, int32 (B,), refreshed per call -- 0 steady, 1 raw-only first frame,
    2 idle -- and its tail launches (v2v_warp_blend_slots, v2v_window_roll_slots) branch on it per stream; everything in front
    of the tail runs for all B streams whatever their mode.
    pool (a _StreamPool): the plan has B = K dense rows and serves K of the pool's S slots: `prev` IS the pool's
    windows, row k works on slot row_slot[k] under row_mode[k] (0 steady, 1 raw-only first frame; int32 (K,), refreshed per call
    like slot_mode).  K == 1 emits the batch-1 body, K > 1 the per-stream one; only the head and the tail know about slots.
    frames_u8: the plan's last launch converts its fake_B rows into `out["image"]`, uint8 (B, H, W, 3) -- (S, H, W, 3)
    for a pool plan -- under the plan's own slot_mode / row_slot words: idle streams and slots come out as zero bytes.
    inputs_u8 (label_nc == 0, plain plans): instead of raw_in the plan owns `win_u8`, the uint8 HWC input window
    (B, tG, H, W, in_ch), and `lut`, fp32 (in_ch, 256); its first launch (Engine.image_prologue) decodes the window into the stem
    input and real_A_last and moves it on by a frame, so a call stages the newest frame only.
    inputs_u8_slots: slot and pool plans take inputs_u8 too.  A slot plan owns win_u8 (B, tG, H, W, in_ch) and its head
    runs under slot_mode (an idle stream's window is not moved on); a pool plan's `win_u8` IS the pool's input windows
    (S, tG, H, W, in_ch), which its K rows reach through row_slot.
    real_A_u8: the plan writes `out["real_A_image"]`, the uint8 input picture (B, H, W, 3) -- (S, H, W, 3) for a pool
    plan -- under the same words as the frames.  Label plans record Engine.label_image on the label maps where real_A_last was
    recorded, and no onehot_planar: `out["real_A_last"]` does not exist.  label_nc == 0 plans convert the first plane(s) of the
    real_A_last they still write, by the frames_u8 launch without normalisation."""

    def __init__(self, model, H, W, in_ch, has_inst, use_raw_only, use_graph=True, u8=False, B=1, slots=False, pool=None,
                 frames_u8=False, inputs_u8=False, real_A_u8=False, inputs_u8_slots=False):
        opt, eng = model.opt, model.engine
        self.model, self.eng = model, eng
        self.H, self.W, self.use_raw_only, self.B = H, W, use_raw_only, B
        self.slots = bool(slots)
        self.frames_u8 = bool(frames_u8)
        self.real_A_u8 = bool(real_A_u8)
        if self.slots and (B < 2 or use_raw_only):
            raise ValueError("a slot plan has B > 1 streams and decides raw-only frames per stream (slot_mode 1)")
        self.pool = pool
        if pool is not None and (self.slots or use_raw_only or not 1 <= B <= pool.S or (pool.H, pool.W) != (H, W)):
            raise ValueError("a pool plan has 1..S rows at the pool's resolution and decides raw-only frames per row (row_mode 1)")
        lead = (B,) if B > 1 else ()
        tG, S = opt.n_frames_G, model.n_scales
        self.label_mode = opt.label_nc != 0
        dev = eng.device
        self.win_u8 = self.lut = self._lut_src = None
        if inputs_u8 and (self.label_mode or ((self.slots or pool is not None) and not inputs_u8_slots)):
            raise ValueError("uint8 image inputs (opt.inputs_u8) go with label_nc == 0 and plain plans")
        # ---- static inputs ----
        if self.label_mode:
            # fp32-encoded integers (the reference loader's format), or uint8 labels + int32 instance ids (SURVEY 8f-2:
            # a quarter of the host-to-device bytes for the label maps; same one-hot / edge tensors bit for bit)
            self.labels = torch.zeros(*lead, tG, H, W, dtype=torch.uint8 if u8 else torch.float32, device=dev)
            self.inst = torch.zeros(*lead, tG, H, W, dtype=torch.int32 if u8 else torch.float32, device=dev) if has_inst else None
            self.raw_in = None
        else:
            self.labels = self.inst = None
            self.raw_in = None if inputs_u8 else torch.zeros(B, tG * in_ch, H, W, dtype=torch.float32, device=dev)
            if inputs_u8:
                self.win_u8 = torch.zeros(B, tG, H, W, in_ch, dtype=torch.uint8, device=dev) if pool is None else \
                    pool.input_windows(in_ch)
                self.lut = torch.zeros(in_ch, 256, dtype=torch.float32, device=dev)
        # fake_B_prev[si]: (tG-1, 3, h, w) per scale, si = 0 finest  (reference :228, :248-250); (B, tG-1, 3, h, w) at B > 1
        if pool is not None:
            self.prev = pool.windows
        else:
            self.prev = [torch.zeros(*lead, tG - 1, opt.output_nc, H >> si, W >> si, dtype=torch.float32, device=dev)
                         for si in range(S)]
        # the plan's int32 words, refreshed per call by set_words: slot_mode (B,) of a slot plan, row_slot | row_mode of a pool plan
        self.slot_mode = self.row_slot = self._words = self._words_host = self._words_copied = None
        self._gather = None              # [pinned host tables, device tables, copy event] of opt.input_geometry calls, at first use
        if self.slots:
            self.slot_mode = self._words = torch.zeros(B, dtype=torch.int32, device=dev)
            # does the finest generator end in the blend launch (which writes an idle stream's row of zeros)?
            self.blend_launch = getattr(model, "netG" + str(S - 1)).blends_in_tail()
        if pool is not None:
            # row_slot | row_mode in one buffer: one 8*K-byte copy per call.  Identity slots until the first call (the warm-up and
            # tuning replays of _build run on valid, distinct slots; _frame_plan puts the windows back behind them)
            self._words = torch.cat([torch.arange(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)]).to(dev)
            self.row_slot, self.slot_mode = self._words[:B], self._words[B:]
            self.dense = {}              # si -> (K, tG-1, 3, h, w): the gathered windows of the paths off the rolling blend
        if self._words is not None:
            self._words_host = torch.zeros(self._words.numel(), dtype=torch.int32)
            if dev.type == "cuda":
                self._words_host = self._words_host.pin_memory()
        self.out = {}
        # independent towers / branches on parallel plan lanes (parallel hipGraph paths); opt.lanes or V2V_LANES
        self.lanes = bool(int(getattr(opt, "lanes", os.environ.get("V2V_LANES", "1")))) and use_graph
        # twin chains (label / image towers, image / flow branches) as paired launches; opt.twin or V2V_TWIN
        self.twin = bool(int(getattr(opt, "twin", os.environ.get("V2V_TWIN", "1"))))
        eng.lanes_enabled = self.lanes
        eng.twin_enabled = self.twin
        eng.per_stream = B > 1          # per-sample statistics for every norm group (BatchNorm2d too) while this plan is emitted
        try:
            self._build(model, opt, eng, use_graph)
        finally:
            eng.lanes_enabled = False
            eng.twin_enabled = False
            eng.per_stream = False

    def _build(self, model, opt, eng, use_graph):
        dev = eng.device
        # warm-up pass sizes the shared scratch, then the same code is recorded
        if not eng.record_only:
            prev_autotune = eng.autotune
            eng.autotune = bool(getattr(opt, "autotune", True))      # per-shape tile selection, measured once
            try:
                self._emit()
            finally:
                eng.autotune = prev_autotune
            torch.cuda.synchronize(dev)
        self._record(use_graph)
        if use_graph and not eng.record_only and self.lanes and bool(int(getattr(opt, "frame_tune", os.environ.get("V2V_FRAME_TUNE", "1")))):
            self._frame_tune(use_graph)

    def _record(self, use_graph):
        eng = self.eng
        self.plan = Plan()
        eng.plan = self.plan
        try:
            with self.plan:
                self._emit()
        finally:
            eng.plan = None
        if use_graph and not eng.record_only:
            self.plan.instantiate_graph()

    def _time_frames(self, n=16, reps=3):
        """Median ms per replay of the current graph (buffers hold whatever they hold: the timing is data independent).
        16 replays per sample: the lane streams start every sample from idle, which costs the first replay ~0.5 ms extra."""
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                self.plan.launch()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / n)
        return sorted(ts)[len(ts) // 2]

    def _frame_tune(self, use_graph, max_trials=160, min_gain=0.005, max_seconds=40.0):
        """Whole-frame tile search.  The per-shape search (Engine._autotune) times every convolution alone on an idle
        chip; inside the frame graph the lanes run beside each other, where e.g. split-K (which fills an idle chip) only
        adds slab traffic.  Greedy pass over the conv shapes of this plan, heaviest first: swap in each runner-up of the
        isolated search, re-record, keep it if the measured frame time drops by more than `min_gain`."""
        eng = self.eng
        work = {}
        for c in self.conv_log:
            k = c.get("tune_key")
            if k in eng._tune_alts and eng._tune_alts[k]:
                work[k] = work.get(k, 0.0) + c["flops"]
        if not work or sum(work.values()) < 5e10:       # nothing to search / toy networks (tests): not worth the trials
            return
        import time
        t_start = time.perf_counter()
        best_ms = self._time_frames()
        base_ms, trials, kept, swaps = best_ms, 0, 0, []
        order = sorted(work, key=lambda kk: -work[kk])

        def trial(k, cand):
            nonlocal best_ms, trials, kept
            prev = eng._tuned[k]
            if tuple(cand) == tuple(prev):
                return
            eng._tuned[k] = tuple(cand)
            try:
                self._emit()                    # eager pass: sizes split-K slabs / statistics rows, packs weights
                torch.cuda.synchronize(eng.device)
                self._record(use_graph)
                ms = self._time_frames()
            except RuntimeError:
                ms = float("inf")
            trials += 1
            if ms < best_ms * (1.0 - min_gain):
                best_ms, kept = ms, kept + 1
                what = ("pair %dx%d k3 s1 @%dx%d" % (k[1], k[2], k[5], k[4])) if k[0] == -2 else \
                       ("%dx%d k%d s%d @%dx%d" % (k[0], k[1], k[2], k[3], k[7], k[6]))
                swaps.append("%s: %s -> %s" % (what, tuple(prev), tuple(cand)))
            else:
                eng._tuned[k] = prev

        def out_of_budget():
            return trials >= max_trials or time.perf_counter() - t_start > max_seconds

        # pass 1: every shape, runners-up of its isolated search; the two heaviest shapes get the wide list
        for rank, k in enumerate(order):
            cands = list(eng._tune_alts[k])
            if rank < 2:
                cands += [c for c in eng._tune_wide.get(k, []) if c not in cands]
            for cand in cands:
                if out_of_budget():
                    break
                trial(k, cand)
        # pass 2: the heaviest shapes again, now beside the other layers' final choices
        for k in order[:3]:
            for cand in eng._tune_alts[k]:
                if out_of_budget():
                    break
                trial(k, cand)
        self._emit()
        torch.cuda.synchronize(eng.device)
        self._record(use_graph)                      # the plan of the final selection
        eng._save_tune_cache()
        self.frame_tune_log = dict(base_ms=round(base_ms, 4), tuned_ms=round(best_ms, 4), trials=trials, kept=kept, swaps=swaps)
        print("frame tune: %.3f -> %.3f ms/frame (%d trials, %d swaps kept)" % (base_ms, best_ms, trials, kept))

    def _emit(self):
        m, eng, opt = self.model, self.eng, self.model.opt
        tG, S = opt.n_frames_G, m.n_scales
        H, W, B = self.H, self.W, self.B
        eng.conv_log = []
        # encode_input (:86-112) + compute_mask (:322-330), fused, straight to NHWC
        if self.label_mode:
            from ..engine import LabelSource
            src = LabelSource(self.labels, self.inst, tG, opt.label_nc)
            netG_fine = getattr(m, "netG" + str(S - 1))
            stems = netG_fine.label_stems() if hasattr(netG_fine, "label_stems") else []
            per_ = opt.label_nc + (1 if self.inst is not None else 0)
            gather = bool(stems) and all(eng.onehot_conv_ok(c, tG * per_, H, W) for c in stems)
            early = gather and os.environ.get("V2V_LABEL_CODES", "1") != "0"     # (A/B switch)
            # one spatial scale, every label stem a gather-sum on the codes: nothing reads the one-hot tensor, and the codes, the
            # foreground mask and the pack of the previous-frame window are one launch (Engine.frame_prologue)
            fused_head = early and S == 1 and opt.label_nc <= 126 and hasattr(netG_fine, "rolls_in_tail")
            if fused_head:
                return self._emit_fused_head(src)
            if B > 1:
                # streams off the fused head (S > 1, stems that are no gather-sums): one encode launch per stream into one
                # batched encoding, the stems as convolutions on it -- correct through the batch-capable kernels, not fast
                early = gather = False
            if early:
                eng.label_codes(src, H, W)                   # one byte per pixel: what the gather-sum stems stage from
            # (writing the one-hot tensor on the foreground tower's lane instead of in front of the towers was measured: -1.5 %,
            # it delays that tower and competes with the label stem; profiles/r02_a29_label_codes_ab.txt)
            x1 = None
            if S > 1 and gather and os.environ.get("V2V_POOLED_ENCODE", "1") != "0":
                # every consumer of the full-resolution encoding reads the label maps itself: it is never written; the first
                # pyramid level comes straight from the maps (537 MB less written and read back per frame at 2048x1024)
                x0, x1, mask0 = eng.encode_labels_pooled(self.labels, self.inst, tG, H, W, opt.label_nc, opt.fg_labels, opt.fg,
                                                         chunk_stride=True, source=src)
            else:
                x0, mask0 = eng.encode_labels(self.labels, self.inst, tG, H, W, opt.label_nc, opt.fg_labels, opt.fg,
                                              chunk_stride=S > 1, source=src)   # fine-scale stems (cout <= 32): LDS-patch 7x7 kernel
        elif self.win_u8 is not None:
            # one spatial scale: the decode, the window pack and (where the generator ends in the blend) the rolls are the head and
            # tail launches, as for label maps
            if S == 1 and not opt.fg and hasattr(m.netG0, "rolls_in_tail"):
                return self._emit_image_head()
            if self.slots or self.pool is not None:
                # (idle streams of a slot plan keep their window; a pool plan's rows work on their slots of the pool's)
                x0, real_last, _, _ = eng.image_prologue(self.win_u8, self.lut, slot_mode=self.slot_mode if self.slots else None,
                                                         row_slot=self.row_slot)
            else:
                x0, real_last, _, _ = eng.image_prologue(self.win_u8, self.lut)
            mask0 = x1 = None
        else:
            x0, mask0, x1 = eng.pack(self.raw_in), None, None
        xs, masks = [x0], [mask0]
        for si in range(1, S):                      # build_pyr of the encoded labels (:205)
            xs.append(x1 if (si == 1 and x1 is not None) else eng.avgpool_nhwc(xs[-1]))
            masks.append(None)
        per = x0.C // tG
        feat = flow_feat = fg_feat = None
        fake_B = None
        for s in range(S):                          # coarse -> fine (:207-208)
            si = S - 1 - s
            netG = getattr(m, "netG" + str(s))
            x = xs[si]
            mask = masks[si]
            if opt.fg and mask is None:
                mask = self._mask_from_pooled(x, per, tG)
            window = self._gathered(si) if self.pool is not None else self.prev[si]
            prev_nchw = window.view(B, -1, H >> si, W >> si)
            fake_B, flow, weight, raw, feat, flow_feat, fg_feat = netG.emit(
                eng, x, eng.pack(prev_nchw), prev_nchw, mask, feat, flow_feat, fg_feat, self.use_raw_only,
                tag="G%d" % s, slot_mode=self.slot_mode)
            # fake_B_prev[si] = cat(prev[1:], fake_B)   (:228)
            self._roll(window, fake_B)
            if self.pool is not None:
                eng.window_scatter(self.prev[si], window, self.row_slot)
            self.out["flow%d" % si], self.out["weight%d" % si], self.out["raw%d" % si] = flow, weight, raw
        self.out["fake_B"] = fake_B
        # real_A[0][0, -1]: encoded last label frame, returned for visualisation (:209)
        if self.label_mode:      # straight from the label map: coalesced planar writes, no NHWC -> NCHW transpose
            self._emit_real_A()
        elif self.win_u8 is not None:      # the prologue decoded the newest frame into planes itself
            self.out["real_A_last"] = real_last[0] if B == 1 else real_last
        else:
            last = Act(x0.t[..., (tG - 1) * per:], per)
            last = eng.unpack(last)
            self.out["real_A_last"] = last[0] if B == 1 else last
        self._emit_input_image()
        self._emit_image()
        self.conv_log = list(eng.conv_log)

    def _emit_real_A(self):
        """Label plans: the planar real_A_last, or with real_A_u8 the picture of it in its place (no planes are written)."""
        if self.real_A_u8:
            opt = self.model.opt
            labels, inst = (self.labels, self.inst) if self.B > 1 else \
                (self.labels.unsqueeze(0), None if self.inst is None else self.inst.unsqueeze(0))
            if self.pool is not None:
                self.out["real_A_image"] = self.eng.label_image(labels, inst, opt.label_nc, self.slot_mode, self.row_slot, S=self.pool.S)
            else:
                self.out["real_A_image"] = self.eng.label_image(labels, inst, opt.label_nc, self.slot_mode if self.slots else None)
        else:
            self.out["real_A_last"] = self._real_A_last()

    def _emit_input_image(self):
        """real_A_u8 plans of label_nc == 0 models: tensor2im(normalize=False) of the first c planes of real_A_last (c = 3 for
        three input channels, else 1, as the reference's test.py picks them), by the launch of the frames."""
        if not self.real_A_u8 or self.label_mode:
            return
        H, W, B = self.H, self.W, self.B
        last = self.out["real_A_last"].view(B, -1, H, W)
        c = 3 if last.shape[1] == 3 else 1
        planes = last[:, :c]
        if not planes.is_contiguous():           # several streams of more planes than the picture takes: its plane of each, densely
            planes = self.eng.empty_f32(B, c, H, W)
            for b in range(B):
                self.eng.memcpy(planes[b], last[b], c * H * W * 4)
        if self.pool is not None:
            self.out["real_A_image"] = self.eng.frames_u8(planes, self.slot_mode, self.row_slot, S=self.pool.S, normalize=False)
        else:
            self.out["real_A_image"] = self.eng.frames_u8(planes, self.slot_mode if self.slots else None, normalize=False)

    def _real_A_last(self):
        """Planar one-hot (+ edge plane) of the newest label frame: (C, H, W), or (B, C, H, W) in one launch at B > 1."""
        tG, opt = self.model.opt.n_frames_G, self.model.opt
        lab = self.labels[tG - 1] if self.B == 1 else self.labels[:, tG - 1]
        inst = None if self.inst is None else (self.inst[tG - 1] if self.B == 1 else self.inst[:, tG - 1])
        return self.eng.onehot_planar(lab, inst, self.H, self.W, opt.label_nc)

    def _emit_fused_head(self, src):
        """The frame at one spatial scale with all label stems on the codes: frame_prologue | towers ... | warp_blend, which
        rolls the window of generated frames itself where the generator ends in it (no device copies behind it).  real_A_last
        depends on the newest label map only: it is emitted behind the foreground tower on that tower's lane, beside the
        ResnetBlock chain, not behind the blend at the frame's tail."""
        m, eng, opt = self.model, self.eng, self.model.opt
        tG, H, W = opt.n_frames_G, self.H, self.W
        netG = m.netG0
        prev = self.prev[0]
        rolls = netG.rolls_in_tail(self.use_raw_only)
        row_slot = None
        if self.pool is not None and rolls:
            # head and tail reach the pool through row_slot: no copy of any window
            row_slot = self.row_slot
            x0, mask0, prev_act, last = eng.frame_prologue(src, H, W, opt.fg_labels, opt.fg, window=prev.view(self.pool.S, -1, H, W),
                                                           last_C=opt.output_nc, row_slot=row_slot)
        else:
            if self.pool is not None:        # no blend launch to roll in: the dense lowering on gathered windows
                prev = self._gathered(0)
            x0, mask0, prev_act, last = eng.frame_prologue(src, H, W, opt.fg_labels, opt.fg, window=prev.view(self.B, -1, H, W),
                                                           last_C=opt.output_nc)

        roll = prev if rolls else None
        fake_B, flow, weight, raw, _, _, _ = netG.emit(eng, x0, prev_act, last, mask0, None, None, None, self.use_raw_only,
                                                       tag="G0", roll=roll, side=self._emit_real_A,
                                                       slot_mode=self.slot_mode, row_slot=row_slot)
        if roll is None:
            self._roll(prev, fake_B)
            if self.pool is not None:
                eng.window_scatter(self.prev[0], prev, self.row_slot)
        self.out["flow0"], self.out["weight0"], self.out["raw0"] = flow, weight, raw
        self.out["fake_B"] = fake_B
        self._emit_image()
        self.conv_log = list(eng.conv_log)

    def _emit_image_head(self):
        """The frame of a uint8-input plan at one spatial scale: image_prologue | towers ... | warp_blend.  The prologue writes
        the stem input, real_A_last, the pack of the generated-frame window and the warp's gather source, and moves the input
        window on; the blend rolls the generated-frame window where the generator ends in it.  No pack, unpack or copy launch.
        Slot plans: the same two launches under slot_mode.  Pool plans: head and tail reach the pool's input and
        generated windows through row_slot where the blend rolls; elsewhere the dense lowering on gathered generated windows."""
        m, eng, opt = self.model, self.eng, self.model.opt
        H, W, B = self.H, self.W, self.B
        netG = m.netG0
        prev = self.prev[0]
        rolls = netG.rolls_in_tail(self.use_raw_only)
        row_slot = None
        if self.pool is not None:
            if rolls:
                row_slot = self.row_slot
                window = prev.view(self.pool.S, -1, H, W)
            else:                            # no blend launch to roll in: the dense lowering on gathered windows
                prev = self._gathered(0)
                window = prev.view(B, -1, H, W)
            x0, real_last, prev_act, last = eng.image_prologue(self.win_u8, self.lut, window=window, last_C=opt.output_nc,
                                                               row_slot=self.row_slot, pooled_window=rolls)
        elif self.slots:
            x0, real_last, prev_act, last = eng.image_prologue(self.win_u8, self.lut, window=prev.view(B, -1, H, W),
                                                               last_C=opt.output_nc, slot_mode=self.slot_mode)
        else:
            x0, real_last, prev_act, last = eng.image_prologue(self.win_u8, self.lut, window=prev.view(B, -1, H, W),
                                                               last_C=opt.output_nc)
        self.out["real_A_last"] = real_last[0] if B == 1 else real_last
        roll = prev if rolls else None
        fake_B, flow, weight, raw, _, _, _ = netG.emit(eng, x0, prev_act, last, None, None, None, None, self.use_raw_only,
                                                       tag="G0", roll=roll, slot_mode=self.slot_mode, row_slot=row_slot)
        if roll is None:
            self._roll(prev, fake_B)
            if self.pool is not None:
                eng.window_scatter(self.prev[0], prev, self.row_slot)
        self.out["flow0"], self.out["weight0"], self.out["raw0"] = flow, weight, raw
        self.out["fake_B"] = fake_B
        self._emit_input_image()
        self._emit_image()
        self.conv_log = list(eng.conv_log)

    def _emit_image(self):
        """frames_u8 plans: the uint8 images of this replay's fake_B rows as the plan's last launch, on the lane that produced them
        (lane 0).  It reads the fake_B buffer whichever launch wrote it, and decides idle rows / slots itself from the plan's words:
        a slot plan's idle rows come out zero also where no blend launch zeroed them, a pool plan's K rows land in its S images."""
        if not self.frames_u8:
            return
        fake_B = self.out["fake_B"]
        fake_B = fake_B.view(self.B, -1, self.H, self.W)
        if self.pool is not None:
            self.out["image"] = self.eng.frames_u8(fake_B, self.slot_mode, self.row_slot, S=self.pool.S)
        else:
            self.out["image"] = self.eng.frames_u8(fake_B, self.slot_mode if self.slots else None)

    def _gathered(self, si):
        """Pool plans off the rolling blend: the windows of this plan's rows at scale si as a dense (K, tG-1, 3, h, w) copy, by
        one launch; the dense lowering runs on it and window_scatter puts it back."""
        dense = self.dense.get(si)
        if dense is None:
            dense = self.dense[si] = torch.zeros((self.B,) + tuple(self.prev[si].shape[1:]), dtype=torch.float32,
                                                 device=self.prev[si].device)
        self.eng.window_gather(dense, self.prev[si], self.row_slot)
        return dense

    def _roll(self, prev, fake_B):
        if self.slots or self.pool is not None:   # one launch under slot_mode: an idle stream's window is not touched
            self.eng.window_roll(prev, fake_B, self.slot_mode)
        elif self.B > 1:                 # (B, tG-1, 3, h, w) <- (B, 3, h, w): every stream rolls its own window
            for b in range(self.B):
                self._roll_one(prev[b], fake_B[b])
        else:
            self._roll_one(prev, fake_B)

    def _roll_one(self, prev, fake_B):
        n = prev.shape[0]
        frame_bytes = prev[0].numel() * 4
        for k in range(n - 1):
            self.eng.memcpy(prev[k], prev[k + 1], frame_bytes)
        self.eng.memcpy(prev[n - 1], fake_B, frame_bytes)

    def _mask_from_pooled(self, x, per, tG):
        # compute_mask on a pooled (fractional) one-hot pyramid level: clamp(sum of fg channels)
        return self.eng.fg_mask(x, (tG - 1) * per, self.model.opt.fg_labels)

    def set_words(self, words):
        """Refresh the plan's words for the next replay -- a slot plan's B modes, a pool plan's K slots followed by its K modes --
        by one asynchronous copy from pinned host memory, like the label buffers.  (The host buffer is rewritten only after the
        previous copy out of it has completed.)"""
        if self._words_copied is not None:
            self._words_copied.synchronize()
        self._words_host.copy_(torch.as_tensor(words, dtype=torch.int32))
        self._words.copy_(self._words_host, non_blocking=True)
        if self._words.device.type == "cuda":
            self._words_copied = torch.cuda.Event()
            self._words_copied.record()

    def gather_tables(self, entries, geoms):
        """The tables of a call's gather launch (opt.input_geometry) in device memory: (entries int32 (E, 4), geoms
        int32 (G, 8)), views of one buffer sized for every frame of the uint8 windows and a geometry per stream.  Like the plan's
        words they are written into pinned host memory and cross by one asynchronous copy; the host buffer is rewritten only after
        the previous copy out of it has completed."""
        streams, frames = self.win_u8.shape[0], self.win_u8.shape[0] * self.win_u8.shape[1]
        if self._gather is None:
            host = torch.zeros(4 * frames + 8 * streams, dtype=torch.int32)
            if self.win_u8.device.type == "cuda":
                host = host.pin_memory()
            self._gather = [host, torch.zeros(host.numel(), dtype=torch.int32, device=self.win_u8.device), None]
        host, dev, copied = self._gather
        if copied is not None:
            copied.synchronize()
        E, G = len(entries), len(geoms)
        host[:4 * E].copy_(torch.tensor(entries, dtype=torch.int32).reshape(-1))
        host[4 * frames:4 * frames + 8 * G].copy_(torch.tensor(geoms, dtype=torch.int32).reshape(-1))
        dev.copy_(host, non_blocking=True)
        if dev.device.type == "cuda":
            self._gather[2] = torch.cuda.Event()
            self._gather[2].record()
        self.gather_last = (dev[:4 * E].view(E, 4), dev[4 * frames:4 * frames + 8 * G].view(G, 8))     # (tests read them)
        return self.gather_last

    def run(self):
        if self.eng.record_only:
            return            # CPU dry run: the plan was validated and recorded, nothing can execute
        self.plan.launch()


class Vid2VidModelG(BaseModel):
    def name(self):
        return "Vid2VidModelG"

    def initialize(self, opt):
        BaseModel.initialize(self, opt)
        self.n_scales = opt.n_scales_spatial
        self.use_single_G = opt.use_single_G
        # reference :37-45: n_gpus_gen < len(gpu_ids) puts G on n_gpus_gen GPUs and D / FlowNet2 on the rest.  With one process per
        # GPU that is a rank-role layout (vid2vid_amd/roles.py, set up by create_model before this runs: opt.gpu_ids is then this
        # rank's own device and opt.role_group_size the reference's GPU count); a single process cannot drive several GPUs here
        self.split_gpus = bool(getattr(opt, "role_group_size", 0))
        if (opt.n_gpus_gen < len(opt.gpu_ids)) and (opt.batchSize == 1) and opt.isTrain:
            raise RuntimeError("n_gpus_gen=%d < %d GPUs selects the generator / discriminator rank roles: launch one process per GPU "
                               "(python -m torch.distributed.run --nproc-per-node %d train.py ...)" % (opt.n_gpus_gen, len(opt.gpu_ids), len(opt.gpu_ids)))

        input_nc = opt.label_nc if opt.label_nc != 0 else opt.input_nc
        netG_input_nc = input_nc * opt.n_frames_G
        if opt.use_instance:
            netG_input_nc += opt.n_frames_G
        prev_output_nc = (opt.n_frames_G - 1) * opt.output_nc
        if opt.openpose_only:
            opt.no_flow = True
        self.netG_input_nc, self.prev_output_nc = netG_input_nc, prev_output_nc

        gpu_ids = self.dev_ids
        self.netG0 = networks.define_G(netG_input_nc, opt.output_nc, prev_output_nc, opt.ngf, opt.netG,
                                       opt.n_downsample_G, opt.norm, 0, gpu_ids, opt)
        for s in range(1, self.n_scales):
            setattr(self, "netG" + str(s),
                    networks.define_G(netG_input_nc, opt.output_nc, prev_output_nc, opt.ngf // (2 ** s),
                                      opt.netG + "Local", opt.n_downsample_G, opt.norm, s, gpu_ids, opt))
        print("---------- Networks initialized -------------")

        if not self.isTrain or opt.continue_train or opt.load_pretrain:
            # opt.use_ema (inference): serve the averaged weights a run with opt.ema_decay saved beside the raw ones
            label = "G%d_ema" if (not self.isTrain and getattr(opt, "use_ema", False)) else "G%d"
            for s in range(self.n_scales):
                self.load_network(getattr(self, "netG" + str(s)), label % s, opt.which_epoch, opt.load_pretrain)
        self.netG_i = self.load_single_G() if self.use_single_G else None
        self._plans = {}
        self._pools = {}

        if self.isTrain:
            self.n_gpus = opt.n_gpus_gen if opt.batchSize == 1 else 1
            self.n_frames_bp = 1
            self.n_frames_per_gpu = min(opt.max_frames_per_gpu, opt.n_frames_total // self.n_gpus)
            self.n_frames_load = self.n_gpus * self.n_frames_per_gpu
            self.old_lr = opt.lr
            self.finetune_all = opt.niter_fix_global == 0
            self._train_coarse = self.finetune_all      # whether gradients reach the coarse scales (base_model.update_fixed_params)
            params = list(getattr(self, "netG" + str(self.n_scales - 1)).parameters())
            if self.finetune_all:
                for s in range(self.n_scales - 1):
                    params += list(getattr(self, "netG" + str(s)).parameters())
            if opt.TTUR:
                beta1, beta2, lr = 0, 0.9, opt.lr / 2
            else:
                beta1, beta2, lr = opt.beta1, 0.999, opt.lr
            ema_decay = float(getattr(opt, "ema_decay", 0.0) or 0.0)
            guard = self.grad_guard_kwargs(opt)          # {} with opt.max_grad_norm / opt.skip_nonfinite_grads off
            if ema_decay > 0.0:
                self.optimizer_G = FusedAdam(params, lr=lr, betas=(beta1, beta2), ema_decay=ema_decay, **guard)
                if opt.continue_train or opt.load_pretrain:
                    self._load_ema(opt)
            else:
                self.optimizer_G = FusedAdam(params, lr=lr, betas=(beta1, beta2), **guard)
        self.bind_precision()

    def _load_ema(self, opt):
        """Resume the averaged weights of each scale from '<epoch>_net_G<s>_ema.pth' where that file exists; a scale without
        one keeps the shadow FusedAdam starts with, a copy of the weights just loaded."""
        views = self.optimizer_G.ema_views()
        for s in range(self.n_scales):
            path = self._ckpt_path("G%d_ema" % s, opt.which_epoch, opt.load_pretrain)
            if not os.path.isfile(path):
                continue
            saved = torch.load(path, map_location="cpu")
            with torch.no_grad():
                for name, p in getattr(self, "netG" + str(s)).named_parameters():
                    if p in views and name in saved and saved[name].shape == p.shape:
                        views[p].copy_(saved[name])

    # ------------------------------------------------------------------ inference
    def _frame_plan(self, H, W, in_ch, has_inst, use_raw_only, u8=False, B=1, slots=False, pool=None, frames_u8=False,
                    inputs_u8=False, real_A_u8=False, inputs_u8_slots=False):
        """pool: the slot capacity S of a pool plan with B rows; its key ends in ("pool", S).
        frames_u8: the plan ends in the uint8 image launch; only then its key gains a field "frames_u8".
        inputs_u8: the plan starts with the uint8 image head; only then its key gains a field "inputs_u8".
        real_A_u8: the plan writes the uint8 input picture; only then its key gains a last field "real_A_u8".
        inputs_u8_slots: a slot or pool plan may have inputs_u8; its key is told apart by the field "inputs_u8"."""
        key = (H, W, in_ch, has_inst, use_raw_only, self.precision, u8, B) + (("slots",) if slots else ()) + \
              ((("pool", pool),) if pool else ()) + (("frames_u8",) if frames_u8 else ()) + (("inputs_u8",) if inputs_u8 else ()) + \
              (("real_A_u8",) if real_A_u8 else ())
        fp = self._plans.get(key)
        if fp is None:
            self.engine.refresh_weights()
            windows = self._stream_pool(pool, H, W) if pool else None
            # building a plan replays it (warm-up, tile search): the live windows are put back behind that
            live = list(windows.windows) if pool else []
            if pool and inputs_u8:               # the uint8 input windows beside them (allocated here at first use)
                live.append(windows.input_windows(in_ch))
            saved = [w.clone() for w in live]
            fp = _FramePlan(self, H, W, in_ch, has_inst, use_raw_only,
                            use_graph=getattr(self.opt, "use_graph", True), u8=u8, B=B, slots=slots, pool=windows,
                            frames_u8=frames_u8, inputs_u8=inputs_u8, real_A_u8=real_A_u8, inputs_u8_slots=inputs_u8_slots)
            for w, keep in zip(live, saved):
                w.copy_(keep)
            self._plans[key] = fp
        return fp

    def _stream_pool(self, S, H, W):
        """The model's windows for S slots at H x W: allocated once, so the plans recorded against them stay valid across restarts."""
        pool = self._pools.get((S, H, W))
        if pool is None:
            pool = self._pools[(S, H, W)] = _StreamPool(S, self.opt.n_frames_G, self.opt.output_nc, H, W, self.n_scales, self.device)
        return pool

    def prepare_streams(self, S, H, W, in_ch, has_inst, u8=False, counts=None):
        """Build the pool plans (opt.compact_streams) of a server with S slots at H x W for the active counts in
        `counts` (default 1..S) ahead of time: each plan records, and searches its tiles, when it is first built -- here rather
        than in the first call that happens to have that many live clips.  in_ch, has_inst, u8: as the calls will have them
        (channels of input_A, whether inst_A is given and used, uint8 label maps).  Activations cost one stream-size per row of
        every plan built: S (S + 1) / 2 stream-sizes for all counts.  The plans are built for opt.frames_u8, opt.real_A_u8 and
        (label_nc == 0) opt.inputs_u8 with opt.inputs_u8_slots as they are now; in_ch is then the last dimension of input_A."""
        counts = list(range(1, S + 1)) if counts is None else sorted(set(int(k) for k in counts))
        if S < 2 or not counts or counts[0] < 1 or counts[-1] > S:
            raise ValueError("prepare_streams: S >= 2 slots and active counts within 1..S")
        in_u8 = bool(self.opt.label_nc == 0 and getattr(self.opt, "inputs_u8", False) and getattr(self.opt, "inputs_u8_slots", False))
        with torch.no_grad():
            for K in counts:
                self._frame_plan(H, W, in_ch, bool(has_inst and self.opt.use_instance and self.opt.label_nc != 0), False, bool(u8),
                                 B=K, pool=S, frames_u8=bool(getattr(self.opt, "frames_u8", False)), inputs_u8=in_u8,
                                 real_A_u8=bool(getattr(self.opt, "real_A_u8", False)), inputs_u8_slots=in_u8)

    @staticmethod
    def _slot_set(arg, B, name):
        """restart= / active= as a list of B bools: a bool mask of shape (B,) or an iterable of stream indices."""
        if isinstance(arg, torch.Tensor):
            arg = arg.detach().cpu()
            is_mask = arg.dtype == torch.bool
            items = arg.reshape(-1).tolist() if arg.dim() <= 1 else None
        else:
            if hasattr(arg, "tolist"):          # numpy arrays
                arg = arg.tolist()
            items = list(arg) if not isinstance(arg, (bool, int)) else None
            is_mask = items is not None and len(items) > 0 and all(isinstance(v, bool) for v in items)
        if items is None:
            raise ValueError("inference: %s is a bool mask of shape (%d,) or an iterable of stream indices" % (name, B))
        if is_mask:
            if len(items) != B:
                raise ValueError("inference: %s mask has %d entries for %d stream(s)" % (name, len(items), B))
            return [bool(v) for v in items]
        flags = [False] * B
        for v in items:
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < B:
                raise ValueError("inference: %s names stream %r, the call has streams 0..%d" % (name, v, B - 1))
            flags[int(v)] = True
        return flags

    def inference(self, input_A, input_B, inst_A, restart=None, active=None):
        """(fake_B (B,3,H,W), real_A_last) for the newest of the tG label frames of each of the B sequences in input_A
        (B,t,c,H,W); inst_A / input_B carry the same leading B.  B == 1: real_A_last is (C,H,W) and model.fake_B_prev a list
        per scale of (tG-1,3,h,w), as in the reference.  B > 1 (multi-stream): real_A_last is (B,C,H,W),
        fake_B_prev a list per scale of (B,tG-1,3,h,w), and stream b gets what a batch-1 model gets on sequence b alone.
        Changing B inside a sequence (fake_B_prev not None) is a ValueError; fake_B_prev = None restarts all streams.
        Stream slots, both a bool mask (B,) or an iterable of stream indices:
        active: the streams that generate a frame in this call (default: all).  An idle stream's rows of the inputs are not
        read, its windows fake_B_prev[si][b] stay bit for bit as they are, its row of fake_B is zero; when it is active again
        it continues where it paused.
        restart: the streams that begin a new sequence with this call: their windows are re-seeded by generate_first_frame on
        their rows alone (input_B rows of the other streams are ignored).  restart implies active; a stream that is restarted
        and idle, an index outside [0, B) or a mask of another length is a ValueError.
        opt.compact_streams (read per call): with B > 1 the call replays a plan with one row per active stream, on
        windows the model owns; the contract above is unchanged.  Setting it while sequences run outside a pool is a ValueError
        (assign fake_B_prev = None with it); clearing it while sequences run continues them, the pool's windows being copied
        once into the slot or plain plan's own.
        opt.frames_u8 (read per call): the first result is `image`, torch.uint8 (B,H,W,output_nc) for every B, instead
        of fake_B: image[b] == visual.tensor2im(fake_B[b]) for every active stream b, fake_B being what the same call returns with
        the option off, and an idle stream's image is all ZERO bytes (not the 127 that zero planes convert to).  The images are
        written by the last launch of the frame plan; real_A_last, fake_B_prev and every other state are as with the option off,
        and the option may change between the calls of running sequences.
        opt.inputs_u8 (read per call; label_nc == 0 only): input_A is torch.uint8 (B,t,H,W,in_ch) -- 8-bit HWC frames as
        a decoder delivers them, on host or device -- with t == n_frames_G, the whole window (required on the first call of a
        sequence, allowed on any), or t == 1, the newest frame alone (only while a sequence started that way is running: the
        plan keeps the older frames and moves them on itself).  The frame plan's first launch decodes byte b of channel c to
        opt.input_lut[c][b] (fp32 (in_ch,256); None: visual.input_lut(in_ch), the reference loader's ToTensor + Normalize); every
        result equals, bit for bit, what the call returns on those decoded fp32 planes with the option off.  Anything else --
        another t, fp32 input_A, a label model, in_ch > 32, a table of another shape, restart= / active= or opt.compact_streams
        (slot and pool plans take fp32 inputs) -- is a ValueError that leaves the running sequences as they are.
        opt.inputs_u8_slots (read per call; has an effect only with opt.inputs_u8): restart=, active= and
        opt.compact_streams are accepted with uint8 inputs.  input_A is uint8 (B,t,H,W,in_ch) with t in {1, n_frames_G}.
        t == n_frames_G is required when the model has no running sequence or when any stream is restarted: a restarted stream
        (on the model's first frame every active one) takes its whole window from its rows, and its first frames come from
        visual.decode_inputs of its rows; every other active stream takes ONLY frame n_frames_G - 1 of its rows -- its older frames
        are not read, a server need not keep them.  t == 1: each active stream takes its newest frame.  An idle stream's rows of
        input_A are not read and its uint8 window stays bit for bit as it is; its row of fake_B / image / real_A_image is zero, its
        row of the fp32 real_A_last is unspecified in a slot plan and zero in a pool plan, as with fp32 inputs.  The uint8 window
        is carried plain <-> slot and pool -> slot (compact_streams cleared) with the generated windows.  A uint8 slot or pool call
        needs no running sequence, or a running plan or pool that holds uint8 windows: a sequence fed with fp32 so far, another t,
        restart together with t == 1 and every other refusal above are ValueErrors raised before any state is touched.  Every
        result for every active stream equals, bit for bit, what the same call schedule returns on the same model with inputs_u8
        off and input_A = visual.decode_inputs(...) as fp32 planes, opt.frames_u8 and opt.real_A_u8 included.
        opt.input_geometry (read per call; with opt.inputs_u8, and opt.inputs_u8_slots for slot and pool calls): input_A
        is uint8 (B,t,Hs,Ws,in_ch) at SOURCE size, on host or device, and the option is the reference's get_img_params dict
        (new_size, crop_size, crop_pos, flip) or a list of B of them, one per stream.  One launch in front of the frame plan writes
        what the reference loader's img.resize(new_size, Image.NEAREST), __crop and flip make of every frame the call brings into
        the plan's uint8 windows -- t = n_frames_G frames of a started or restarted stream, the newest frame of every other active
        one, nothing of an idle one; the rules for t are those above.  (H, W) of the call is visual.geometry_size of the
        geometries, which must agree with each other and with the running sequences.  Every result equals, bit for bit, the same
        call with the option off on frames resized that way on the host.  The option without opt.inputs_u8 or on a label model, a
        list of another length, sizes that differ, new_size or source sizes outside 1..16384, a crop_pos outside the resized frame
        and a flip that is no bool are ValueErrors raised before anything is staged or launched.
        opt.real_A_u8 (read per call): the second result is `real_A_image`, a fresh torch.uint8 tensor, instead of the
        fp32 real_A_last.  Label models: (B,H,W,3) for every B, real_A_image[b] == visual.tensor2label(real_A_last[b], opt.label_nc)
        bit for bit, real_A_last being what the same call returns with the option off; one launch of the frame plan writes it from
        the label map and the instance map, and the one-hot planes are never made.  label_nc == 0: (B,H,W,c), c = 3 for three
        input channels and 1 otherwise, real_A_image[b] == visual.tensor2im(real_A_last[b][:c], normalize=False) with its channel
        dimension kept.  An idle stream's picture is all zero bytes.  The first result, fake_B_prev and every other state are as
        with the option off; it combines with every option and argument above and may change between the calls of running
        sequences."""
        opt = self.opt
        tG = opt.n_frames_G
        with torch.no_grad():
            in_u8 = bool(getattr(opt, "inputs_u8", False))
            lut = geo = None
            if getattr(opt, "input_geometry", None) is not None and (not in_u8 or opt.label_nc != 0):
                raise ValueError("inference: opt.input_geometry goes with opt.inputs_u8 on an image model (label_nc == 0); "
                                 "visual.resample_u8 resizes label maps")
            if in_u8:
                lut = self._check_inputs_u8(input_A, restart, active)
                geo = self._check_input_geometry(input_A)
                B, t_in, H, W, in_ch = input_A.shape
                if geo is not None:                  # input_A is at source size; the model's size is the geometry's
                    H, W = geo[:2]
            else:
                B, t_in, in_ch, H, W = input_A.shape
                if t_in < tG:
                    raise ValueError("inference needs n_frames_G=%d label frames, got %d" % (tG, t_in))
            for name, t in (("inst_A", inst_A if opt.use_instance else None), ("input_B", input_B)):
                if t is not None and t.shape[0] != B:
                    raise ValueError("inference: input_A holds %d sequence(s), %s %d" % (B, name, t.shape[0]))
            slot_call = restart is not None or active is not None
            if slot_call:
                act = [True] * B if active is None else self._slot_set(active, B, "active")
                rst = [False] * B if restart is None else self._slot_set(restart, B, "restart")
                both = [b for b in range(B) if rst[b] and not act[b]]
                if both:
                    raise ValueError("inference: stream(s) %s are restarted and idle in the same call" % both)
            self._check_device_status()
            self.is_first_frame = not hasattr(self, "fake_B_prev") or self.fake_B_prev is None
            if not self.is_first_frame and self._active_plan is not None:
                running = self._active_plan.B if self._active_plan.pool is None else self._active_plan.pool.S
                if running != B:
                    raise ValueError("inference: %d sequence(s) given while %d are running; assign fake_B_prev = None to restart"
                                     % (B, running))
            has_inst = bool(opt.use_instance and inst_A is not None and opt.label_nc != 0)
            img = bool(getattr(opt, "frames_u8", False))
            pic = bool(getattr(opt, "real_A_u8", False))
            if slot_call and B == 1:
                # one stream needs no slot plan: idle is no call at all, a restart is fake_B_prev = None
                if not act[0]:
                    last_C = in_ch if opt.label_nc == 0 else opt.label_nc + int(has_inst)
                    idle = torch.zeros(1, H, W, opt.output_nc, dtype=torch.uint8, device=self.device) if img else \
                        torch.zeros(1, opt.output_nc, H, W, dtype=torch.float32, device=self.device)
                    if pic:
                        return idle, torch.zeros(1, H, W, self._picture_channels(in_ch), dtype=torch.uint8, device=self.device)
                    return idle, torch.zeros(last_C, H, W, dtype=torch.float32, device=self.device)
                if rst[0]:
                    self.fake_B_prev = None
                    self.is_first_frame = True
                slot_call = False
            if self.is_first_frame:
                self._slots_on = False
            if slot_call:
                self._slots_on = True            # sticky until fake_B_prev = None
            u8 = bool(opt.label_nc != 0 and input_A.dtype == torch.uint8)
            if B > 1 and getattr(opt, "compact_streams", False):
                if not slot_call:
                    act, rst = [True] * B, [False] * B
                return self._inference_pool(input_A, input_B, inst_A, act, rst, has_inst, u8, img, pic, lut, geo)
            if self._slots_on:
                if not slot_call:
                    act, rst = [True] * B, [False] * B
                return self._inference_slots(input_A, input_B, inst_A, act, rst, has_inst, u8, img, pic, lut, geo)
            use_raw_only = bool(opt.no_first_img and self.is_first_frame)
            fp = self._frame_plan(H, W, in_ch, has_inst, use_raw_only, u8, B, frames_u8=img, inputs_u8=in_u8, real_A_u8=pic)
            if not in_u8:
                self._stage_inputs(fp, input_A, inst_A, has_inst, list(range(B)))
            if self.is_first_frame:
                # (uint8 inputs: the first-frame generators read fp32 planes -- decoded once per sequence, off the hot path)
                from ..visual import decode_inputs
                if geo is not None:      # ... of the frames at model size: the gather launch goes first and they read its window
                    self._stage_inputs_geometry(fp, input_A, lut, list(range(B)), list(range(B)), geo)
                    planes = decode_inputs(fp.win_u8, lut)
                else:
                    planes = decode_inputs(input_A.to(self.device), lut) if in_u8 else input_A
                self._seed_windows(fp.prev, planes, input_B, inst_A)
            else:
                self._carry_windows(fp)                                          # e.g. first-frame plan -> steady plan
            if geo is not None:
                if not self.is_first_frame:
                    self._stage_inputs_geometry(fp, input_A, lut, list(range(B)), list(range(B)) if t_in == tG else [], geo)
            elif in_u8:                  # behind the carry: the newest frame lands in the window the sequence has reached
                self._stage_inputs_u8(fp, input_A, lut)
            self._active_plan = fp
            self.fake_B_prev = fp.prev
            fp.run()
            # fresh tensors per frame, as the reference returns them (the plan's output buffers are overwritten by the
            # next replay; a caller collecting a clip must not see every entry alias the last frame)
            return fp.out["image" if img else "fake_B"].clone(), fp.out["real_A_image" if pic else "real_A_last"].clone()

    def _picture_channels(self, in_ch):
        """Channels of real_A_image (opt.real_A_u8): the palette's 3 for label maps; for images 3 of three input channels, else 1."""
        return 3 if self.opt.label_nc != 0 or in_ch == 3 else 1

    def _stage_inputs(self, fp, input_A, inst_A, has_inst, rows, in_place=False):
        """Stage (H2D or D2D) the newest tG frames of the streams `rows` (ascending) into fp's static buffers; the other streams'
        rows of the inputs are not read.  Pinned host tensors copy asynchronously.
        in_place False: they become the plan's rows 0..len(rows)-1, by one copy per tensor (plain and pool plans).
        in_place True: stream b is row b of the plan (slot plans) -- one copy per tensor when every stream is named, else per row."""
        tG, dev = self.opt.n_frames_G, self.device
        every = len(rows) == input_A.shape[0] > 1
        if in_place and not every:
            pairs = [(b, b) for b in rows]                                   # (rows of the inputs, rows of the plan)
        else:
            pairs = [(slice(None) if every else rows[0] if len(rows) == 1 else rows, Ellipsis)]
        for src, dst in pairs:
            if fp.label_mode:
                fp.labels[dst].copy_(input_A[src, :tG, 0].to(dev, fp.labels.dtype, non_blocking=True))
                if has_inst:
                    fp.inst[dst].copy_(inst_A[src, :tG, 0].to(dev, fp.inst.dtype, non_blocking=True))
            else:
                raw = fp.raw_in[dst]
                raw.copy_(input_A[src, :tG].reshape(raw.shape).to(dev, torch.float32, non_blocking=True))

    def _input_table(self, in_ch):
        """opt.input_lut as a device tensor, or the default table of in_ch channels (built once)."""
        lut = getattr(self.opt, "input_lut", None)
        if lut is None:
            cache = self.__dict__.setdefault("_default_luts", {})
            if in_ch not in cache:
                from ..visual import input_lut
                cache[in_ch] = input_lut(in_ch).to(self.device)
            return cache[in_ch]
        if not isinstance(lut, torch.Tensor) or lut.dtype != torch.float32 or tuple(lut.shape) != (in_ch, 256):
            raise ValueError("inference: opt.input_lut is an fp32 tensor (%d, 256): one row per channel of input_A" % in_ch)
        return lut

    def _check_inputs_u8(self, input_A, restart, active):
        """Every refusal of a call with opt.inputs_u8, before the call touches any state; returns the table of the call."""
        opt, tG = self.opt, self.opt.n_frames_G
        if opt.label_nc != 0:
            raise ValueError("inference: opt.inputs_u8 is for image inputs (label_nc == 0); label maps are uint8 already")
        if not isinstance(input_A, torch.Tensor) or input_A.dtype != torch.uint8 or input_A.dim() != 5:
            raise ValueError("inference: with opt.inputs_u8 input_A is torch.uint8 (B, t, H, W, in_ch)")
        B, t_in, _, _, in_ch = input_A.shape
        if in_ch > 32:
            raise ValueError("inference: opt.inputs_u8 decodes at most 32 input channels, input_A has %d" % in_ch)
        running = hasattr(self, "fake_B_prev") and self.fake_B_prev is not None
        if getattr(opt, "inputs_u8_slots", False):
            self._check_inputs_u8_slots(input_A, restart, active, running)
        else:
            if restart is not None or active is not None:
                raise ValueError("inference: restart= / active= (slot plans) take fp32 inputs; opt.inputs_u8 runs plain plans only")
            if B > 1 and getattr(opt, "compact_streams", False):
                raise ValueError("inference: opt.compact_streams (pool plans) takes fp32 inputs; opt.inputs_u8 runs plain plans only")
            if running and self._slots_on:
                raise ValueError("inference: the running sequences are in a slot plan, which takes fp32 inputs")
        if t_in not in (1, tG):
            raise ValueError("inference: with opt.inputs_u8 input_A holds the whole window (t = %d) or the newest frame (t = 1), "
                             "got t = %d" % (tG, t_in))
        if t_in == 1 and tG > 1 and not (running and self._active_plan is not None and self._active_plan.win_u8 is not None):
            raise ValueError("inference: the newest frame alone (t = 1) continues a sequence that a whole uint8 window started")
        return self._input_table(in_ch)

    def _check_inputs_u8_slots(self, input_A, restart, active, running):
        """opt.inputs_u8_slots: what a uint8 call with restart= / active= / opt.compact_streams, or one that continues
        a slot plan, needs beyond _check_inputs_u8's rules -- checked, like them, before the call touches any state."""
        opt, tG = self.opt, self.opt.n_frames_G
        B, t_in = input_A.shape[:2]
        rst = restart is not None and any(self._slot_set(restart, B, "restart"))
        if rst and t_in != tG:
            raise ValueError("inference: a restarted stream takes its whole uint8 window (t = %d), got t = %d" % (tG, t_in))
        slot_call = B > 1 and (restart is not None or active is not None or bool(getattr(opt, "compact_streams", False))
                               or (running and self._slots_on))
        if slot_call and running and (self._active_plan is None or self._active_plan.win_u8 is None):
            raise ValueError("inference: the running sequences were fed fp32 inputs; a uint8 slot or pool call continues uint8 "
                             "windows (assign fake_B_prev = None to restart)")

    def _stage_inputs_u8_slots(self, fp, input_A, lut, rows, new):
        """uint8 inputs of a slot or pool plan: stream b's window is fp.win_u8[b] (the slot plan's own, or the pool's).  The
        streams in `new` take their whole window from their rows; every other stream of `rows` (the active ones, ascending) takes
        the newest frame of its rows alone, into slot tG - 1 of the window the plan has moved on.  One copy when every stream is
        active (_stage_inputs' rule), else one per active row; the idle streams' rows are not read."""
        tG, win = self.opt.n_frames_G, fp.win_u8
        if fp._lut_src is not lut:
            fp.lut.copy_(lut)
            fp._lut_src = lut
        if len(rows) == win.shape[0]:
            if len(new) == len(rows):
                win.copy_(input_A, non_blocking=True)
                return
            win[:, tG - 1].copy_(input_A[:, -1], non_blocking=True)
        else:
            for b in rows:
                if b not in new:
                    win[b, tG - 1].copy_(input_A[b, -1], non_blocking=True)
        for b in new:
            win[b].copy_(input_A[b], non_blocking=True)

    def _stage_inputs_u8(self, fp, input_A, lut):
        """uint8 inputs: the whole window, or the newest frame into slot tG - 1 of the window the plan has moved on itself."""
        tG = self.opt.n_frames_G
        if fp._lut_src is not lut:
            fp.lut.copy_(lut)
            fp._lut_src = lut
        if input_A.shape[1] == tG:
            fp.win_u8.copy_(input_A, non_blocking=True)
        else:
            fp.win_u8[:, tG - 1].copy_(input_A[:, 0], non_blocking=True)

    def _check_input_geometry(self, input_A):
        """opt.input_geometry of a call that _check_inputs_u8 has let through: None with the option off, else (H, W,
        geoms) -- the model-side size every stream's geometry yields and the int32 rows [new_w, new_h, x1, y1, flip, 0, 0, 0] of
        the launch's table, one for a dict, B for a list.  Every refusal is raised here, before the call touches any state."""
        from ..visual import geometry_words, GEOMETRY_MAX_SIZE
        geometry = getattr(self.opt, "input_geometry", None)
        if geometry is None:
            return None
        B, _, Hs, Ws, _ = input_A.shape
        if not (1 <= Hs <= GEOMETRY_MAX_SIZE and 1 <= Ws <= GEOMETRY_MAX_SIZE):
            raise ValueError("inference: opt.input_geometry takes source frames of 1..%d rows and columns, input_A has %dx%d"
                             % (GEOMETRY_MAX_SIZE, Ws, Hs))
        per_stream = isinstance(geometry, (list, tuple))
        if per_stream and len(geometry) != B:
            raise ValueError("inference: opt.input_geometry lists %d geometries for %d stream(s)" % (len(geometry), B))
        words = [geometry_words(g) for g in (geometry if per_stream else [geometry])]
        H, W = words[0][5:]
        for b, w in enumerate(words):
            if tuple(w[5:]) != (H, W):
                raise ValueError("inference: opt.input_geometry gives stream %d frames of %dx%d, stream 0 of %dx%d: one plan runs "
                                 "one size" % (b, w[6], w[5], W, H))
        running = getattr(self, "fake_B_prev", None) is not None and self._active_plan is not None
        if running and (self._active_plan.H, self._active_plan.W) != (H, W):
            raise ValueError("inference: opt.input_geometry gives frames of %dx%d, the running sequences are at %dx%d; assign "
                             "fake_B_prev = None to restart" % (W, H, self._active_plan.W, self._active_plan.H))
        return H, W, [list(w[:5]) + [0, 0, 0] for w in words]

    def _stage_inputs_geometry(self, fp, input_A, lut, rows, new, geo):
        """uint8 inputs at source size (opt.input_geometry): ONE launch (Engine.gather_frames_u8) resizes, crops and
        flips every frame the call brings into fp.win_u8 -- the plan's own windows or the pool's, stream b's window being
        win_u8[b].  The streams in `new` send their whole window, every other stream of `rows` (the active ones, ascending) its
        newest frame into slot tG - 1 of the window the plan has moved on; the idle streams' rows are not read.  Frames on the
        host cross first, and only those the launch reads."""
        from ..visual import gather_entries
        tG, dev = self.opt.n_frames_G, self.device
        if fp._lut_src is not lut:
            fp.lut.copy_(lut)
            fp._lut_src = lut
        B, t_in = input_A.shape[:2]
        entries = gather_entries(t_in, tG, rows, new, len(geo[2]) > 1)
        if not entries:
            return
        if input_A.device != dev:
            src = torch.empty(input_A.shape, dtype=torch.uint8, device=dev)
            if len(rows) == B and (len(new) == B or t_in == 1):
                src.copy_(input_A, non_blocking=True)
            else:
                for b in rows:
                    if b in new:
                        src[b].copy_(input_A[b], non_blocking=True)
                    else:
                        src[b, -1].copy_(input_A[b, -1], non_blocking=True)
        else:
            src = input_A.contiguous()
        tables = fp.gather_tables(entries, geo[2])
        self.engine.gather_frames_u8(src, fp.win_u8, *tables)

    def _seed_windows(self, windows, input_A, input_B, inst_A, new=None, lut=None):
        """Seed `windows` (a list per scale) from generate_first_frame: whole (new=None: the first frame of every sequence), or
        the streams in the list `new` alone, from their rows of the inputs alone (windows then have a leading stream dimension).
        lut: input_A is uint8 HWC and the first-frame generators get visual.decode_inputs of the rows they read."""
        if new is None:
            first = self.generate_first_frame(input_A, input_B, inst_A)         # list per scale (tG-1,3,h,w) / (B,tG-1,3,h,w)
        elif new:
            rows_A = input_A[new]
            if lut is not None:
                from ..visual import decode_inputs
                rows_A = decode_inputs(rows_A.to(self.device), lut)
            first = self.generate_first_frame(rows_A, None if input_B is None else input_B[new],
                                              None if inst_A is None else inst_A[new])
        else:
            return
        for si in range(self.n_scales):
            if new is None:
                windows[si].copy_(first[si])
            else:
                for k, b in enumerate(new):
                    windows[si][b].copy_(first[si] if len(new) == 1 else first[si][k])

    def _carry_windows(self, fp):
        """fp continues the running sequences: unless it ran last itself, it gets the windows of the plan that did."""
        if self._active_plan is not fp:
            for si in range(self.n_scales):
                fp.prev[si].copy_(self._active_plan.prev[si])
            if fp.win_u8 is not None and self._active_plan.win_u8 is not None:      # the uint8 input window, as far as it has moved
                fp.win_u8.copy_(self._active_plan.win_u8)

    def _inference_slots(self, input_A, input_B, inst_A, act, rst, has_inst, u8, img=False, pic=False, lut=None, geo=None):
        """One replay of the slot plan (B > 1).  act / rst: B bools.  On the first frame of the model
        (fake_B_prev = None) every active stream starts a sequence and the windows of the idle ones are zero.
        img (opt.frames_u8): the uint8 images the plan's last launch wrote, idle rows zero, instead of fake_B.
        pic (opt.real_A_u8): the uint8 input pictures the plan wrote, idle rows zero, instead of real_A_last.
        lut (opt.inputs_u8 with opt.inputs_u8_slots): input_A is uint8 (B,t,H,W,in_ch) and this is the call's table.
        geo (opt.input_geometry): _check_input_geometry's result; input_A is at source size and one gather launch
        stages it -- ahead of the first-frame generators, which then read a restarted stream's window at model size."""
        opt = self.opt
        in_u8 = lut is not None
        if in_u8:
            B, _, H, W, in_ch = input_A.shape
        else:
            B, _, in_ch, H, W = input_A.shape
        if geo is not None:
            H, W = geo[:2]
        fp = self._frame_plan(H, W, in_ch, has_inst, False, u8, B, slots=True, frames_u8=img, inputs_u8=in_u8, real_A_u8=pic,
                              inputs_u8_slots=in_u8)
        if self.is_first_frame:
            rst = list(act)
        # the rows of the active streams, each in its place (the buffers keep an idle stream's last valid rows)
        rows = [b for b in range(B) if act[b]]
        new = [b for b in range(B) if rst[b]]
        if not in_u8:
            self._stage_inputs(fp, input_A, inst_A, has_inst, rows, in_place=True)
        if self.is_first_frame:
            for si in range(self.n_scales):
                fp.prev[si].zero_()
            if in_u8:
                fp.win_u8.zero_()
        else:
            self._carry_windows(fp)                                              # plain plan -> slot plan
        if geo is not None:              # behind the carry, ahead of the seeding, which reads the gathered windows
            self._stage_inputs_geometry(fp, input_A, lut, rows, new, geo)
            self._seed_windows(fp.prev, fp.win_u8, input_B, inst_A, new, lut)
        else:
            self._seed_windows(fp.prev, input_A, input_B, inst_A, new, lut)
            if in_u8:                    # behind the carry: into the windows the sequences have reached
                self._stage_inputs_u8_slots(fp, input_A, lut, rows, new)
        fp.set_words([2 if not act[b] else (1 if (rst[b] and opt.no_first_img) else 0) for b in range(B)])
        self._active_plan = fp
        self.fake_B_prev = fp.prev
        fp.run()
        real_A = fp.out["real_A_image" if pic else "real_A_last"].clone()
        if img:                  # the image launch zeroed the idle rows itself, with or without a blend launch in front of it
            return fp.out["image"].clone(), real_A
        fake = fp.out["fake_B"].clone()
        if not fp.blend_launch and len(rows) != B:        # no blend launch in this generator: nothing wrote the idle rows' zeros
            fake[[b for b in range(B) if not act[b]]] = 0
        return fake, real_A

    def _inference_pool(self, input_A, input_B, inst_A, act, rst, has_inst, u8, img=False, pic=False, lut=None, geo=None):
        """One call of a compacting model (opt.compact_streams, B = S > 1 slots): the contract of _inference_slots,
        by a replay of the pool plan that has one row per ACTIVE stream -- row k runs slot rows[k], rows ascending.
        img (opt.frames_u8): the plan's last launch delivers the (S,H,W,3) uint8 images, idle slots zero; no zero tensor and no
        indexed copy for the frames.
        pic (opt.real_A_u8): the same for the second result, the (S,H,W,3) uint8 input pictures.
        lut (opt.inputs_u8 with opt.inputs_u8_slots): input_A is uint8 (S,t,H,W,in_ch), staged into the pool's uint8
        input windows, slot b's rows into window b; the plan's rows reach them through row_slot.
        geo (opt.input_geometry): _check_input_geometry's result; input_A is at source size and one gather launch
        writes slot b's frames into window b."""
        opt, dev = self.opt, self.device
        in_u8 = lut is not None
        if in_u8:
            S, _, H, W, in_ch = input_A.shape
        else:
            S, _, in_ch, H, W = input_A.shape
        if geo is not None:
            H, W = geo[:2]
        rows = [b for b in range(S) if act[b]]
        K = len(rows)
        last_C = in_ch if opt.label_nc == 0 else opt.label_nc + int(has_inst)
        if not img:
            fake = torch.zeros(S, opt.output_nc, H, W, dtype=torch.float32, device=dev)
        elif K == 0:
            fake = torch.zeros(S, H, W, opt.output_nc, dtype=torch.uint8, device=dev)
        if not pic:
            real_A_last = torch.zeros(S, last_C, H, W, dtype=torch.float32, device=dev)
        elif K == 0:
            real_A_last = torch.zeros(S, H, W, self._picture_channels(in_ch), dtype=torch.uint8, device=dev)
        if K == 0:                      # nothing is live: no replay, no state touched
            return fake, real_A_last
        pool = self._stream_pool(S, H, W)
        if not self.is_first_frame and (self._active_plan is None or self._active_plan.pool is not pool):
            raise ValueError("inference: the running sequences are not in a %d-slot pool at %dx%d; assign fake_B_prev = None "
                             "to restart" % (S, W, H))
        fp = self._frame_plan(H, W, in_ch, has_inst, False, u8, B=K, pool=S, frames_u8=img, inputs_u8=in_u8, real_A_u8=pic,
                              inputs_u8_slots=in_u8)
        if self.is_first_frame:
            rst = list(act)
            for w in pool.windows:
                w.zero_()
            if in_u8:
                fp.win_u8.zero_()
        new = [b for b in range(S) if rst[b]]
        if geo is not None:
            self._stage_inputs_geometry(fp, input_A, lut, rows, new, geo)  # the active streams' frames, resized into their windows
        elif in_u8:
            self._stage_inputs_u8_slots(fp, input_A, lut, rows, new)      # the active streams' rows, each into its slot's window
        else:
            self._stage_inputs(fp, input_A, inst_A, has_inst, rows)       # the active streams' rows, straight into the dense rows
        self._seed_windows(pool.windows, fp.win_u8 if geo is not None else input_A, input_B, inst_A, new, lut)
        fp.set_words(rows + [1 if (rst[b] and opt.no_first_img) else 0 for b in rows])
        pool.idle = [b for b in range(S) if not act[b]]
        self._active_plan = fp
        self.fake_B_prev = pool.windows
        fp.run()
        # one indexed copy of the dense rows into the zero tensors: fresh tensors per frame, idle rows zero
        index = fp.row_slot.long()
        if img:
            fake = fp.out["image"].clone()
        else:
            fake.index_copy_(0, index, fp.out["fake_B"])
        if pic:
            return fake, fp.out["real_A_image"].clone()
        last = fp.out["real_A_last"]
        real_A_last.index_copy_(0, index, last if K > 1 else last.unsqueeze(0))
        return fake, real_A_last

    def _check_device_status(self):
        """Kernels cannot return errors; the library's host-visible status word says whether a fused-norm spin barrier of
        an EARLIER frame gave up (another process held compute units: its workgroups were not all co-resident).  That
        frame's outputs are NaN.  Detected here, the engine falls back to the unfused norm (separate bn_apply launches: no
        barrier, no co-residency requirement), the frame plans are dropped so that the next call re-records them without
        it, and the caller gets an error instead of silently poisoned frames (ADVICE r2 / VERDICT r2 item 13)."""
        from ..lib import lib
        if lib.v2v_device_status(0) & 1:
            lib.v2v_device_status(1)
            self.engine.fused_norm = False
            self._plans.clear()
            self._active_plan = None
            self.fake_B_prev = None
            raise RuntimeError("a fused-norm barrier timed out on the device (is another process using this GPU?): the last "
                               "frame(s) are invalid.  The model has switched to the unfused norm (V2V_FUSED_NORM=0) and reset "
                               "its sequence state; restart the sequence.")

    def generate_first_frame(self, input_A, input_B, inst_A=None):
        """Pyramid of the tG-1 frames that precede the first generated one (reference :231-251)."""
        opt = self.opt
        tG = opt.n_frames_G
        B, _, _, H, W = input_A.shape
        dev = self.device
        if opt.no_first_img:
            first = torch.zeros(B, tG - 1, opt.output_nc, H, W, dtype=torch.float32, device=dev)
        elif opt.isTrain or opt.use_real_img:
            if input_B is None:
                raise ValueError("use_real_img needs the first real frames (input_B)")
            first = input_B[:, :tG - 1].to(dev, torch.float32)
        elif opt.use_single_G and getattr(opt, "dataset_mode", "temporal") == "face":
            # reference :239-244 with dataset_mode == 'face': raw input maps + feature map of the given real frame; the
            # pooling map is the instance map (encode_input :104-106)
            if input_B is None or inst_A is None:
                raise ValueError("the face first-frame generator needs the first real frames and the part map")
            frames = []
            for i in range(tG - 1):
                feat_map = self.get_face_features(input_B[:, i], inst_A[:, i])
                frames.append(self.netG_i.forward(input_A[:, i].to(dev, torch.float32), feat_map).unsqueeze(1))
            first = torch.cat(frames, dim=1)
        elif opt.use_single_G:
            eng = self.engine
            seqs = []
            for b in range(B):                # the single-image generator runs once per sequence
                frames = []
                lab = input_A[b, :, 0].to(dev, torch.float32).contiguous()
                for i in range(tG - 1):       # one-hot labels only, no edge channel (reference :239-244)
                    onehot, _ = eng.encode_labels(lab[i:i + 1], None, 1, H, W, opt.label_nc, (), False)
                    frames.append(self.netG_i.emit(eng, onehot).unsqueeze(1))
                seqs.append(torch.cat(frames, dim=1))
            first = seqs[0] if B == 1 else torch.cat(seqs, dim=0)
        else:
            raise ValueError("Please specify the method for generating the first frame")
        pyr = self.build_pyr(first.contiguous())
        return [p[0] for p in pyr] if B == 1 else list(pyr)

    def load_single_G(self):
        """First-frame single-image generator (reference :261-288).  Only the Cityscapes nets are on
        the hot path; their checkpoints are external downloads, so a missing file is an error unless
        opt.random_init_ok."""
        import os
        opt = self.opt
        gpu_ids = self.dev_ids
        if "City" in opt.dataroot:
            base = "checkpoints/label2city_single/"
            if opt.loadSize == 512:
                path, netG = base + "latest_net_G_512.pth", networks.define_G(35, 3, 0, 64, "global", 3, "instance", 0, gpu_ids, opt)
            elif opt.loadSize == 1024:
                path, netG = base + "latest_net_G_1024.pth", networks.define_G(35, 3, 0, 64, "global", 4, "instance", 0, gpu_ids, opt)
            elif opt.loadSize == 2048:
                path, netG = base + "latest_net_G_2048.pth", networks.define_G(35, 3, 0, 32, "local", 4, "instance", 0, gpu_ids, opt)
            else:
                raise ValueError("Single image generator does not exist")
        elif "face" in opt.dataroot:                    # reference :277-284 (edge2face: feature-encoding generator + encoder)
            base = "checkpoints/edge2face_single/"
            opt.feat_num = 16
            path, netG = base + "latest_net_G.pth", networks.define_G(15, 3, 0, 64, "global_with_features", 3, "instance", 0, gpu_ids, opt)
            self.netE = networks.define_G(3, 16, 0, 16, "encoder", 4, "instance", 0, gpu_ids, opt)
            epath = base + "latest_net_E.pth"
            if os.path.isfile(epath):
                self.netE.load_state_dict(torch.load(epath, map_location="cpu"))
            elif not getattr(opt, "random_init_ok", False):
                raise RuntimeError("%s not found" % epath)
            self.face_features_path = base + "features.npy"
        else:
            raise ValueError("Single image generator does not exist")
        if os.path.isfile(path):
            netG.load_state_dict(torch.load(path, map_location="cpu"))
        elif not getattr(opt, "random_init_ok", False):
            raise RuntimeError("%s not found" % path)
        return netG

    def get_face_features(self, real_image, inst):
        """reference :290-320: encoder features of the given real frame, replaced per facial part by those of the nearest
        training image (checkpoints/edge2face_single/features.npy, an external download like the checkpoints)."""
        import os
        import numpy as np
        if not os.path.isfile(self.face_features_path):
            raise RuntimeError("%s not found (feature dictionary of the edge2face single-image model)" % self.face_features_path)
        features = np.load(self.face_features_path, encoding="latin1", allow_pickle=True).item()
        dev = self.device
        feat_map = self.netE.forward(real_image.to(dev, torch.float32), inst.to(dev, torch.float32))
        return nearest_face_features(feat_map, inst.to(dev, torch.float32), features, self.opt.feat_num)

    # ------------------------------------------------------------------ training
    def encode_input(self, input_map, real_image=None, inst_map=None):
        """One-hot labels + instance edges as the planar (B,T,C,H,W) tensor the reference returns
        (reference :86-112); produced by the fused NHWC encoder + one layout pass, never by scatter_."""
        opt, eng, dev = self.opt, self.engine, self.device
        B, T, _, H, W = input_map.shape
        if opt.label_nc != 0:
            per = opt.label_nc + (1 if (opt.use_instance and inst_map is not None) else 0)
            outs = []
            for b in range(B):
                lab = input_map[b, :, 0].to(dev, torch.float32).contiguous()
                inst = inst_map[b, :, 0].to(dev, torch.float32).contiguous() if per != opt.label_nc else None
                with torch.no_grad():
                    x, _ = eng.encode_labels(lab, inst, T, H, W, opt.label_nc, (), False)
                    outs.append(eng.unpack(x).view(1, T, per, H, W))
            real_A = outs[0] if B == 1 else torch.cat(outs, 0)
        else:
            real_A = input_map.to(dev, torch.float32)
            if opt.use_instance and inst_map is not None:
                real_A = torch.cat([real_A, self.get_edges(inst_map.to(dev, torch.float32))], dim=2)
        real_B = None if real_image is None else real_image.to(dev, torch.float32)
        return real_A, real_B, None

    def forward(self, input_A, input_B, inst_A, fake_B_prev, dummy_bs=0, frame_range=None, first_chunk=None):
        """n_frames_load frames with autograd (reference :114-137).  Returns the reference's 7-tuple.
        frame_range=(t0, t1) (roles.py, a generator rank of a sequence group): only frames t0..t1-1 of the chunk, `fake_B_prev`
        being the tG-1 frames just before t0; fake_B / fake_B_raw / flow / weight then hold t1-t0 frames.  first_chunk: whether the
        chunk opens a sequence (`--no_first_img` makes ALL its frames raw-only, reference :160); a generator rank behind the first
        one receives its previous frames and cannot tell from `fake_B_prev is None`."""
        tG = self.opt.n_frames_G
        if dummy_bs:
            input_A, input_B, inst_A, fake_B_prev = [None if t is None else t[dummy_bs:] for t in
                                                     (input_A, input_B, inst_A, fake_B_prev)]
        # (packed weight copies follow the optimizer lazily: Engine.packed() refreshes the one a launch reads)
        real_A_all, real_B_all, _ = self.encode_input(input_A, input_B, inst_A)
        networks.note_inputs_ready(real_B_all)       # FlowNet2 (called next by train.py, on these frames) need not wait for the generator
        self.bs = real_A_all.shape[0]
        is_first_frame = fake_B_prev is None
        if is_first_frame:
            with torch.no_grad():
                fake_B_prev = self._first_frames_train(real_A_all, real_B_all)
        if first_chunk is not None:
            is_first_frame = bool(first_chunk)
        fake_B, fake_B_raw, flow, weight = self.generate_frame_train(real_A_all, list(fake_B_prev), is_first_frame, frame_range)
        fake_B_prev = [B[:, -tG + 1:].detach() for B in fake_B]
        fake_B = [B[:, tG - 1:] for B in fake_B]
        return fake_B[0], fake_B_raw, flow, weight, real_A_all[:, tG - 1:], real_B_all[:, tG - 2:], fake_B_prev

    def _first_frames_train(self, real_A_all, real_B_all):
        """Pyramid (finest first) of the tG-1 frames preceding the first generated one, (B,tG-1,3,h,w)."""
        opt, tG = self.opt, self.opt.n_frames_G
        B, _, _, H, W = real_A_all.shape
        if opt.no_first_img:
            first = torch.zeros(B, tG - 1, opt.output_nc, H, W, dtype=torch.float32, device=self.device)
        else:                       # isTrain: the real frames (reference :236-238)
            first = real_B_all[:, :tG - 1].contiguous()
        return self.build_pyr(first)

    def generate_frame_train(self, real_A_all, fake_B_pyr, is_first_frame, frame_range=None):
        """Frame-sequential, coarse-to-fine generation with the reference's detach rules (:139-196)."""
        opt, eng = self.opt, self.engine
        tG, S = opt.n_frames_G, self.n_scales
        with torch.no_grad():
            real_A_pyr = self.build_pyr(real_A_all.contiguous())
        per = real_A_all.shape[2]
        fake_Bs_raw = flows = weights = None
        t0, t1 = (0, self.n_frames_load) if frame_range is None else frame_range
        for t in range(t0, t1):
            feat = flow_feat = fg_feat = None
            lt = t - t0                                # index into fake_B_pyr, which starts tG-1 frames before frame t0
            for s in range(S):
                si = S - 1 - s
                real_As = real_A_pyr[si]
                _, _, _, h, w = real_As.shape
                x = eng.pack(real_As[:, t:t + tG].reshape(self.bs, -1, h, w).contiguous())
                prevs = fake_B_pyr[si][:, lt:lt + tG - 1]
                if (t % self.n_frames_bp) == 0:
                    prevs = prevs.detach()
                prev_nchw = prevs.reshape(self.bs, -1, h, w).contiguous()
                mask = eng.fg_mask(x, (tG - 1) * per, opt.fg_labels) if opt.fg else None
                use_raw_only = bool(opt.no_first_img and is_first_frame)
                netG = getattr(self, "netG" + str(s))
                fake_B, flow, weight, fake_B_raw, feat, flow_feat, fg_feat = netG.emit(
                    eng, x, eng.pack(prev_nchw), prev_nchw, mask, feat, flow_feat, fg_feat, use_raw_only, tag="G%d" % s)
                if s != S - 1 and not getattr(self, "_train_coarse", self.finetune_all):       # train the finest scale only (:181-186)
                    fake_B, feat = fake_B.detach(), feat.detach()
                    if flow is not None:
                        flow, flow_feat = flow.detach(), flow_feat.detach()
                    if fg_feat is not None:
                        fg_feat = fg_feat.detach()
                fake_B_pyr[si] = self.concat([fake_B_pyr[si], fake_B.unsqueeze(1)], dim=1)
                if s == S - 1:
                    fake_Bs_raw = self.concat([fake_Bs_raw, fake_B_raw.unsqueeze(1)], dim=1)
                    if flow is not None:
                        flows = self.concat([flows, flow.unsqueeze(1)], dim=1)
                        weights = self.concat([weights, weight.unsqueeze(1)], dim=1)
        return fake_B_pyr, fake_Bs_raw, flows, weights

    # ------------------------------------------------------------------ helpers used by train.py
    def compute_mask(self, real_As, ts, te=None):
        if te is None:
            te = ts + 1
        mask_F = real_As[:, ts:te, self.opt.fg_labels[0]].clone()
        for i in range(1, len(self.opt.fg_labels)):
            mask_F = mask_F + real_As[:, ts:te, self.opt.fg_labels[i]]
        return torch.clamp(mask_F, 0, 1)

    def compute_fake_B_prev(self, real_B_prev, fake_B_last, fake_B):
        fake_B_prev = real_B_prev[:, 0:1] if fake_B_last is None else fake_B_last[0][:, -1:]
        if fake_B.size()[1] > 1:
            fake_B_prev = torch.cat([fake_B_prev, fake_B[:, :-1].detach()], dim=1)
        return fake_B_prev

    def save(self, label):
        for s in range(self.n_scales):
            self.save_network(getattr(self, "netG" + str(s)), "G" + str(s), label, self.gpu_ids)
        # averaged weights (opt.ema_decay): '<label>_net_G<s>_ema.pth' for every scale the STEPPING optimizer holds --
        # after the reference-compatible update_fixed_params that is _optimizer_G_live, not the stand-in in optimizer_G
        live = getattr(self, "_optimizer_G_live", getattr(self, "optimizer_G", None))
        if getattr(live, "ema_decay", 0.0) > 0.0:
            views = live.ema_views()
            for s in range(self.n_scales):
                net = getattr(self, "netG" + str(s))
                if any(p in views for p in net.parameters()):
                    torch.save(live.ema_state_dict(net), self._ckpt_path("G%d_ema" % s, label))

    _active_plan = None
    _slots_on = False
