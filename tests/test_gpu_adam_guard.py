"""The gradient guard of the fused Adam step on the GPU: v2v_grad_sumsq / v2v_adam_step_dev_guard(_ema) against
torch's fp64 norm, against the formula of the scale word, against the UNGUARDED entry points (bit contracts: the reference of
every update is v2v_adam_step_dev / v2v_adam_step_dev_ema, never the new kernels), skipped steps, graph replay, the side
stream, torch's clip_grad_norm_ + Adam, and through the models (opt.max_grad_norm / opt.skip_nonfinite_grads)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest
import torch
import torch.nn as nn

from util import assert_close, sd_from_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
PAD = 8                                   # guard floats in front of and behind every buffer
HYPER = dict(lr=2e-4, b1=0.5, b2=0.999, eps=1e-8)
HEAD = struct.Struct("<dfiiiif")          # include/v2v_hip.h: norm_sq, scale, skip, skipped, nonfinite, applied, gscale
# 4*256*3+5: three workgroups and a tail; the last: more than 1024 workgroups x 256 threads x 4 floats, so every partial is
# written and the grid-stride loop runs
SIZES = [1, 3, 255, 257, 4 * 256 * 3 + 5, 2 ** 20 + 2 ** 18 + 7]
BIG = SIZES[-1]
OFFS = [0, 1, 3]                          # floats off 16-byte alignment: the scalar head has 0, 3 and 1 elements


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _new_guard():
    from vid2vid_amd.lib import lib
    return torch.zeros(int(lib.v2v_adam_guard_workspace_bytes()) // 4, dtype=torch.int32, device=DEV)


def _head(guard):
    return dict(zip(("norm_sq", "scale", "skip", "skipped", "nonfinite", "applied", "gscale"),
                    HEAD.unpack(guard[:HEAD.size // 4].cpu().numpy().tobytes())))


class Bufs:
    """param, grad, exp_avg, exp_avg_sq (>= 0), ema: seeded normals, each a window of n floats that starts `off` floats behind a
    16-byte boundary, inside an allocation with guard floats around it."""
    names = ("p", "g", "m", "v", "e")

    def __init__(self, n, seed=0, off=0, like=None):
        self.n, self.o = n, 4 + off
        if like is None:
            gen = torch.Generator(device=DEV).manual_seed(seed)
            vals = [torch.randn(n, device=DEV, generator=gen) for _ in range(5)]
            vals[3] = vals[3] * vals[3]
        else:
            vals = [like.win(k) for k in self.names]
        self.full = {}
        for k, val in zip(self.names, vals):
            t = torch.full((n + 2 * PAD,), 12345.0, device=DEV)
            t[self.o:self.o + n] = val
            self.full[k] = t
        assert self.win("g").data_ptr() % 16 == (4 * off) % 16

    def win(self, k):
        return self.full[k][self.o:self.o + self.n]

    def guards_intact(self):
        return all(bool((t[:self.o] == 12345.0).all()) and bool((t[self.o + self.n:] == 12345.0).all()) for t in self.full.values())

    def same(self, other, keys=("p", "m", "v", "e")):
        return all(torch.equal(self.win(k).view(torch.int32), other.win(k).view(torch.int32)) for k in keys)


def _state(step=0):
    host = torch.zeros(2, dtype=torch.int32)
    host[0] = step
    host[1:2].view(torch.float32)[0] = HYPER["lr"]
    return host.to(DEV)


def _parent(b, state, wd, gs, decay=None):
    """The unguarded device-state entry points: the reference of every update below."""
    from vid2vid_amd.lib import lib, check
    h = HYPER
    if decay is None:
        check(lib.v2v_adam_step_dev(_ptr(b.win("p")), _ptr(b.win("g")), _ptr(b.win("m")), _ptr(b.win("v")), b.n,
                                    h["b1"], h["b2"], h["eps"], wd, gs, _ptr(state), _stream()), "adam_step_dev")
    else:
        check(lib.v2v_adam_step_dev_ema(_ptr(b.win("p")), _ptr(b.win("g")), _ptr(b.win("m")), _ptr(b.win("v")), _ptr(b.win("e")), b.n,
                                        h["b1"], h["b2"], h["eps"], wd, gs, _ptr(state), decay, _stream()), "adam_step_dev_ema")


def _guarded(b, state, guard, wd, gs, max_norm, skip, decay=None):
    from vid2vid_amd.lib import lib, check
    h = HYPER
    if decay is None:
        check(lib.v2v_adam_step_dev_guard(_ptr(b.win("p")), _ptr(b.win("g")), _ptr(b.win("m")), _ptr(b.win("v")), b.n,
                                          h["b1"], h["b2"], h["eps"], wd, gs, _ptr(state), _ptr(guard), max_norm, int(skip),
                                          _stream()), "adam_step_dev_guard")
    else:
        check(lib.v2v_adam_step_dev_guard_ema(_ptr(b.win("p")), _ptr(b.win("g")), _ptr(b.win("m")), _ptr(b.win("v")),
                                              _ptr(b.win("e")), b.n, h["b1"], h["b2"], h["eps"], wd, gs, _ptr(state), decay,
                                              _ptr(guard), max_norm, int(skip), _stream()), "adam_step_dev_guard_ema")


def _sumsq(g, guard):
    from vid2vid_amd.lib import lib, check
    check(lib.v2v_grad_sumsq(_ptr(g), g.numel(), _ptr(guard), _stream()), "grad_sumsq")


def _ref_norm_sq(g):
    """torch, fp64, on the CPU."""
    return float(g.detach().cpu().double().pow(2).sum())


# --------------------------------------------------------------------------------------------------------------- 1. norm
# the last size: 4 x (1024 workgroups x 256 threads) float4 and more, so the loop that keeps four loads in flight runs too
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", SIZES + [4 * 2 ** 20 + 2 ** 19 + 5])
def test_norm_sq_against_torch_fp64(n, off):
    """Both sums add non-negative fp64 terms (a float squared is exact in fp64), so each is within (n - 1) * 2^-53 relative of
    the exact sum whatever its order: the two differ by at most 2 * n * 2^-53 relative.  Derived, not measured."""
    b = Bufs(n, seed=n + off, off=off)
    guard = _new_guard()
    for huge in (False, True):
        g = b.win("g")
        if huge:
            g[n // 2] = -1e30                           # finite in fp32, its square is not: the kernel has to square in fp64
        _sumsq(g, guard)
        h1 = _head(guard)
        raw1 = guard[:2].clone()
        _sumsq(g, guard)
        assert torch.equal(guard[:2], raw1), "two runs on the same data give equal bits"
        ref = _ref_norm_sq(g)
        rel = abs(h1["norm_sq"] - ref) / ref
        print("n=%d off=%d huge=%d: norm_sq %.17g, torch %.17g, rel diff %.3e (bound %.3e)" % (n, off, huge, h1["norm_sq"], ref, rel,
                                                                                                2 * n * 2.0 ** -53))
        assert np.isfinite(h1["norm_sq"]) and h1["nonfinite"] == 0
        assert rel <= 2 * n * 2.0 ** -53
        assert h1["scale"] == 1.0 and h1["skip"] == 0 and h1["skipped"] == 0 and h1["applied"] == 0
        if huge:
            assert h1["norm_sq"] >= 1e60
    assert b.guards_intact()


# --------------------------------------------------------------------------------------------------------- 2. scale word
@pytest.mark.parametrize("gs", [1.0, 0.25])
@pytest.mark.parametrize("n,off", [(3, 1), (257, 0), (4 * 256 * 3 + 5, 3)])
def test_scale_word_is_the_fp64_formula_rounded_once(n, off, gs):
    """scale = (float)(gscale * min(1, max_norm / (gscale * sqrt(norm_sq) + 1e-6))) evaluated on the host in fp64 from torch's
    fp64 norm: the kernel's fp64 value differs from it by ~n * 2^-53 relative, then one rounding to fp32 (2^-24); bound 2^-23."""
    b = Bufs(n, seed=5 * n, off=off)
    total = gs * _ref_norm_sq(b.win("g")) ** 0.5
    for frac in (2.0, 0.5, 1e-4):                       # clamp at 1, about 0.5, about 1e-4
        max_norm = float(np.float32(frac * total))      # the value the C ABI receives
        guard = _new_guard()
        _guarded(Bufs(n, off=off, like=b), _state(0), guard, 0.0, gs, max_norm, False)
        h = _head(guard)
        want = gs * min(1.0, max_norm / (total + 1e-6))
        rel = abs(h["scale"] - want) / want
        print("n=%d gs=%g frac=%g: scale %.9g, formula %.17g, rel diff %.3e" % (n, gs, frac, h["scale"], want, rel))
        assert rel <= 2.0 ** -23
        if frac == 2.0:
            assert h["scale"] == gs, "a clamp of 1 leaves gscale's bits"
        assert h["gscale"] == gs and h["skip"] == 0 and h["applied"] == 1
    guard = _new_guard()
    _guarded(Bufs(n, off=off, like=b), _state(0), guard, 0.0, gs, 0.0, True)
    assert _head(guard)["scale"] == gs, "max_norm = 0: clipping is off"


# ------------------------------------------------------------------------------------- 3. the update is the parent's update
@pytest.mark.parametrize("shadow", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (0.01, 1.0), (0.0, 0.25), (0.01, 0.25)])
@pytest.mark.parametrize("n", SIZES)
def test_guarded_update_has_the_bits_of_the_unguarded_entry_points(n, wd, gs, shadow):
    decay = 0.9 if shadow else None
    keys = ("p", "m", "v", "e") if shadow else ("p", "m", "v")
    for off in OFFS:
        src = Bufs(n, seed=3 * n + off, off=off)
        total = gs * float(src.win("g").double().norm())
        # clipped: the unguarded entry point with grad_scale = the scale word read back
        new, old = Bufs(n, off=off, like=src), Bufs(n, off=off, like=src)
        sn, so, guard = _state(2), _state(2), _new_guard()
        _guarded(new, sn, guard, wd, gs, 0.5 * total, True, decay)
        h = _head(guard)
        assert h["skip"] == 0 and h["nonfinite"] == 0 and 0.0 < h["scale"] < gs
        _parent(old, so, wd, h["scale"], decay)
        assert new.same(old, keys), "clipped step, n=%d off=%d" % (n, off)
        assert not torch.equal(new.win("p"), src.win("p")), "the step did run"
        assert torch.equal(sn, so) and int(sn[0]) == 3 and h["applied"] == 3
        if not shadow:
            assert torch.equal(new.win("e"), src.win("e"))
        assert new.guards_intact()
        # nothing clips: the plain step with the caller's own gscale
        new, old = Bufs(n, off=off, like=src), Bufs(n, off=off, like=src)
        sn, so = _state(2), _state(2)
        _guarded(new, sn, guard, wd, gs, 1e30, True, decay)
        assert _head(guard)["scale"] == gs
        _parent(old, so, wd, gs, decay)
        assert new.same(old, keys) and torch.equal(sn, so), "unclipped step, n=%d off=%d" % (n, off)
        assert new.guards_intact()


# --------------------------------------------------------------------------------------------------------------- 4. skip
# (n, off, index): index 0, n - 1, inside the scalar head of an offset buffer (off = 1: a head of three), and -- the last size
# only -- an index that a thread reaches in its SECOND grid-stride pass (beyond 1024 x 256 float4)
_POISON_AT = [(1, 0, 0), (257, 0, 0), (257, 3, 256), (257, 1, 2), (BIG, 1, 0), (BIG, 1, BIG - 1), (BIG, 1, 2),
              (BIG, 0, 4 * (1024 * 256 + 1000) + 1)]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("n,off,idx", _POISON_AT)
def test_nonfinite_gradient_skips_the_step_and_the_next_step_never_knew(n, off, idx, bad):
    for decay in (None, 0.9):
        src = Bufs(n, seed=n + idx, off=off)
        b, twin = Bufs(n, off=off, like=src), Bufs(n, off=off, like=src)
        st, st_twin, guard, guard_twin = _state(4), _state(4), _new_guard(), _new_guard()
        clean = b.win("g").clone()
        b.win("g")[idx] = bad
        _guarded(b, st, guard, 0.01, 0.5, 1.0, True, decay)
        h = _head(guard)
        assert h["skip"] == 1 and h["skipped"] == 1 and h["nonfinite"] >= 1 and h["applied"] == 4
        assert b.same(src) and int(st[0]) == 4 and torch.equal(st, _state(4)), "nothing moved"
        # the next step, on clean gradients, is the step of an optimizer that never saw the bad one
        b.win("g").copy_(clean)
        _guarded(b, st, guard, 0.01, 0.5, 1.0, True, decay)
        _guarded(twin, st_twin, guard_twin, 0.01, 0.5, 1.0, True, decay)
        h = _head(guard)
        assert h["skip"] == 0 and h["skipped"] == 1 and h["nonfinite"] == 0 and h["applied"] == 5
        assert b.same(twin) and torch.equal(st, st_twin) and not b.same(src, ("p",))
        assert b.guards_intact()
    # skip_nonfinite off, clipping on: the value propagates as torch's clip_grad_norm_ lets it; the guard reports it
    b = Bufs(n, off=off, like=src)
    b.win("g")[idx] = bad
    st = _state(4)
    _guarded(b, st, guard, 0.0, 1.0, 1.0, False)
    h = _head(guard)
    assert h["nonfinite"] >= 1 and h["skip"] == 0 and h["skipped"] == 1 and int(st[0]) == 5


# ------------------------------------------------------------------------------------------------ 5. / 6. the optimizer
def _twin_optimizers(capturable=False, count=2, **kw):
    from vid2vid_amd.optim import FusedAdam
    torch.manual_seed(41)
    shapes = [(7, 5, 3, 3), (13,), (4, 9)]
    base = [torch.randn(*s) for s in shapes]
    out = []
    for _ in range(count):
        ps = [nn.Parameter(t.clone().to(DEV)) for t in base]
        opt = FusedAdam(ps, lr=2e-4, betas=(0.5, 0.999), **kw)
        if capturable:
            opt.make_capturable()
        out.append(opt)
    return out


def _same_optimizer_state(a, b):
    return (torch.equal(a.flat.flat_param, b.flat.flat_param) and torch.equal(a.exp_avg, b.exp_avg)
            and torch.equal(a.exp_avg_sq, b.exp_avg_sq) and torch.equal(a.ema, b.ema))


def _fills(numel, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    grads = [torch.randn(numel, device=DEV, generator=gen) * 3.0 for _ in range(3)]
    grads[1][numel // 3] = float("nan")                   # clean, poisoned, clean
    return grads


def test_guarded_step_replays_in_a_graph():
    """A guarded step captured once with torch.cuda.graph and replayed over a clean, a poisoned and a clean gradient: the
    decision is taken on the device at every replay, so the state equals an eager guarded optimizer's, two updates were applied
    and one skipped."""
    kw = dict(ema_decay=0.9, max_grad_norm=1.0, skip_nonfinite=True)
    graphed, eager = _twin_optimizers(**kw)
    assert graphed.capturable and eager.capturable, "a guarded optimizer keeps its state on the device"
    warm = _twin_optimizers(count=1, **kw)[0]
    warm.step()                                           # the three kernels have run once before anything is captured
    grads = _fills(graphed.flat.numel, 9)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    p0 = graphed.flat.flat_param.clone()
    with torch.cuda.graph(g):
        graphed.step()
    assert graphed.device_step() == 0 and torch.equal(graphed.flat.flat_param, p0), "capture launches nothing"
    for k, gr in enumerate(grads):
        graphed.flat.flat_grad.copy_(gr); g.replay()
        eager.flat.flat_grad.copy_(gr); eager.step()
        assert graphed.guard_stats() == eager.guard_stats() or k == 1     # (NaN != NaN in the poisoned step's norm)
    torch.cuda.synchronize()
    assert _same_optimizer_state(graphed, eager) and not torch.equal(graphed.flat.flat_param, p0)
    assert graphed.device_step() == 2 and eager.device_step() == 2
    s = graphed.guard_stats()
    assert s["skipped"] == 1 and s["applied"] == 2 and s["nonfinite"] == 0 and s["clip_coef"] < 1.0
    assert graphed.state_dict()["skipped"] == 1 and graphed.state_dict()["step"] == 2


def test_overlapped_guarded_step_runs_on_the_side_stream():
    """GradSync.run_overlapped (a world-size-1 RCCL group with the collective forced on): the three launches run on the side
    stream behind the all-reduce; guard_stats() waits for them by itself and the results equal a non-overlapped optimizer's."""
    import socket
    import torch.distributed as dist
    from vid2vid_amd import parallel
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        oa, ob = _twin_optimizers(ema_decay=0.9, max_grad_norm=1.0, skip_nonfinite=True)
        gs = parallel.sync_optimizers([oa], bucket_bytes=1 << 10, force_collective=True)
        for it, gr in enumerate(_fills(oa.flat.numel, 10)):
            oa.zero_grad(); ob.zero_grad()
            oa.flat.flat_grad.copy_(gr); ob.flat.flat_grad.copy_(gr)
            oa.step(); ob.step()
            assert gs.pending(oa)
            sa = oa.guard_stats()                         # waits for the pending step by itself
            assert not gs.pending(oa)
            if it != 1:
                assert sa == ob.guard_stats(), it
            else:
                assert sa["nonfinite"] == 1 and sa["skipped"] == 1
        torch.cuda.synchronize()
        assert _same_optimizer_state(oa, ob)
        assert oa.device_step() == 2 and oa.guard_stats() == ob.guard_stats() and oa.guard_stats()["skipped"] == 1
    finally:
        parallel._ACTIVE_SYNCS.clear()
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------ 7. what users write today
def test_clipped_fused_adam_matches_clip_grad_norm_and_torch_adam():
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on a CPU copy, 5 steps, every step clipped (the gradients' norm is
    ~70, max_norm 1).  torch takes the norm in fp32 and rescales the gradient in a pass of its own, so this is a tolerance test,
    at the tolerance test_fused_adam_matches_torch (tests/test_gpu_train_ops.py) uses for the unclipped comparison: 1e-6 per
    element relative to |ref| + rms(ref).  Measured: 3.7e-8 at most, so the wider bar from torch's own fp32-vs-fp64 clipped run
    was not needed."""
    from vid2vid_amd.optim import FusedAdam
    torch.manual_seed(33)
    shapes = [(16, 12, 3, 3), (40,), (33, 29)]
    ref_p = [nn.Parameter(torch.randn(*s)) for s in shapes]
    dev_p = [nn.Parameter(p.detach().clone().to(DEV)) for p in ref_p]
    ref_opt = torch.optim.Adam(ref_p, lr=2e-4, betas=(0.5, 0.999))
    opt = FusedAdam(dev_p, lr=2e-4, betas=(0.5, 0.999), max_grad_norm=1.0)
    for it in range(5):
        grads = [torch.randn(*s) * (1.0 + it) for s in shapes]
        ref_opt.zero_grad(); opt.zero_grad()
        for p, g in zip(ref_p, grads):
            p.grad = g.clone()
        for p, g in zip(dev_p, grads):
            p.grad.add_(g.to(DEV))
        total = torch.nn.utils.clip_grad_norm_(ref_p, 1.0)
        ref_opt.step(); opt.step()
        s = opt.guard_stats()
        assert abs(s["grad_norm"] - float(total)) <= 1e-5 * float(total) and s["clip_coef"] < 0.1
    assert opt.device_step() == 5
    for p, q in zip(dev_p, ref_p):
        e = assert_close(p.detach().cpu(), q.detach(), 1e-6, "clipped adam parameter")
        print("clipped adam vs torch: per-element relative error %.3e" % e)


# ---------------------------------------------------------------------------------------------------------- 8. model level
def _train_models(g, ckpt, **kw):
    """The golden training configuration (tests/golden/training_label2city_s2_32x64.npz's shapes and weights)."""
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models.vid2vid_model_G import Vid2VidModelG
    from vid2vid_amd.models.vid2vid_model_D import Vid2VidModelD
    opt = make_opt(isTrain=True, label_nc=35, loadSize=64, use_instance=True, fg=True, ngf=8, n_blocks=2,
                   n_blocks_local=1, n_scales_spatial=2, n_downsample_G=2, no_vgg=True, num_D=2, ndf=8,
                   n_frames_total=6, max_frames_per_gpu=3, n_scales_temporal=1, niter_fix_global=0,
                   precision="fp32", gpu_ids=[0], random_init_ok=True, checkpoints_dir=ckpt, name="guard", **kw)
    G = Vid2VidModelG(); G.initialize(opt)
    D = Vid2VidModelD(); D.initialize(opt)
    G.netG0.load_state_dict(sd_from_npz(g, "sdG0."))
    G.netG1.load_state_dict(sd_from_npz(g, "sdG1."))
    D.netD.load_state_dict(sd_from_npz(g, "sdD."))
    D.netD_T0.load_state_dict(sd_from_npz(g, "sdDT0."))
    if kw.get("ema_decay"):
        G.optimizer_G.seed_ema()                          # the weights were replaced behind the optimizer's back
    return opt, G, D


def _optimizers(G, D):
    return {"optimizer_G": G.optimizer_G, "optimizer_D": D.optimizer_D, "optimizer_D_T0": D.optimizer_D_T0}


def _train(g, G, D, n_chunks, before_G_step=None):
    """train.py:50-95 per chunk with the fixture's flow_ref / conf_ref standing in for FlowNet2; returns, per chunk, the flat
    weights of the three optimizers and the models' grad_guard_stats()."""
    lab, inst, Bimg = T(g["in.labels"]).to(DEV), T(g["in.inst"]).to(DEV), T(g["in.B"]).to(DEV)
    flow_ref, conf_ref = T(g["in.flow_ref"]).to(DEV), T(g["in.conf_ref"]).to(DEV)
    reshape = lambda ts: [None if t is None else t.contiguous().view(-1, t.size(2), t.size(3), t.size(4)) for t in ts]
    weights, stats = [], []
    for chunk in range(n_chunks):
        fake_B, fake_B_raw, flow, weight, real_A, real_Bp, fake_B_last = G(lab, Bimg, inst, None)
        real_B_prev, real_B = real_Bp[:, :-1], real_Bp[:, 1:]
        fake_B_prev = G.compute_fake_B_prev(real_B_prev, None, fake_B)
        losses = D(0, reshape([real_B, fake_B, fake_B_raw, real_A, real_B_prev, fake_B_prev, flow, weight, flow_ref, conf_ref]))
        loss_dict = dict(zip(D.loss_names, [torch.mean(x) for x in losses]))
        _, skipped = D.get_all_skipped_frames((None,) * 4, real_B, fake_B, flow_ref, conf_ref, 1, 3, G.n_frames_load, 0, None)
        lt = D(1, [f[0] for f in skipped])
        loss_dict_T = [dict(zip(D.loss_names_T, [torch.mean(x) for x in lt]))]
        loss_G, loss_D, loss_D_T, _ = D.get_losses(loss_dict, loss_dict_T, 1)
        G.optimizer_G.zero_grad(); loss_G.backward()
        if before_G_step is not None:
            before_G_step(chunk)
        G.optimizer_G.step()
        D.optimizer_D.zero_grad(); loss_D.backward(); D.optimizer_D.step()
        D.optimizer_D_T0.zero_grad(); loss_D_T[0].backward(); D.optimizer_D_T0.step()
        torch.cuda.synchronize()
        weights.append({k: o.flat.flat_param.clone() for k, o in _optimizers(G, D).items()})
        stats.append(dict(G.grad_guard_stats(), **D.grad_guard_stats()))
    return weights, stats


_BASE = {}


def _baseline(golden, tmp_path):
    """Shared by the three model tests, computed once: a throw-away chunk (the engine picks and keeps a tile for every shape of
    this configuration), then the run with both options OFF and its optimizers in device-state mode, and the guarded run (a)."""
    if not _BASE:
        g = golden("training_label2city_s2_32x64")
        ck = str(tmp_path)
        _, G, D = _train_models(g, ck)
        _train(g, G, D, 1)
        _BASE["pinned"] = dict(G.engine._tuned)
        _, G, D = _train_models(g, ck)
        for o in _optimizers(G, D).values():
            assert not hasattr(o, "_guard") and not o.capturable
            o.make_capturable()
        _BASE["off"], stats = _train(g, G, D, 2)
        assert stats == [{}, {}]
        _, G, D = _train_models(g, ck, skip_nonfinite_grads=True, max_grad_norm=1e30)
        _BASE["on"], _BASE["on_stats"] = _train(g, G, D, 2)
        _BASE["g"] = g
        assert dict(G.engine._tuned) == _BASE["pinned"], "a tile was searched between the compared runs"
    return _BASE


def test_model_with_an_idle_guard_trains_the_same_weights(golden, tmp_path):
    """(a) skip_nonfinite_grads with max_grad_norm = 1e30: nothing skips, nothing clips, every weight of the three optimizers is
    torch.equal to the run with the options off.  The off run's optimizers are make_capturable()'d: a guarded optimizer is in
    device-state mode, and the parent's device-state form evaluates the bias corrections with the device's pow(), the
    host-step form with the host's -- those two forms of the parent are not promised to agree in bits."""
    base = _baseline(golden, tmp_path)
    for k, (off, on) in enumerate(zip(base["off"], base["on"])):
        for name in off:
            assert torch.equal(off[name], on[name]), "%s after chunk %d differs from the run without the guard" % (name, k)
    assert not torch.equal(base["on"][0]["optimizer_G"], base["on"][1]["optimizer_G"])
    for k, stats in enumerate(base["on_stats"]):
        assert sorted(stats) == ["optimizer_D", "optimizer_D_T0", "optimizer_G"]
        for name, s in stats.items():
            assert s["skipped"] == 0 and s["clip_coef"] == 1.0 and s["nonfinite"] == 0 and s["applied"] == k + 1, (name, s)
            assert 0.0 < s["grad_norm"] < float("inf")


def test_model_clips_below_the_reported_norm(golden, tmp_path):
    """(b) max_grad_norm at half the smallest norm any optimizer reported in chunk 1 of (a): every optimizer clips in chunk 1,
    the weights leave (a)'s, training runs on and saves."""
    base = _baseline(golden, tmp_path)
    g, ck = base["g"], str(tmp_path)
    max_norm = 0.5 * min(s["grad_norm"] for s in base["on_stats"][0].values())
    _, G, D = _train_models(g, ck, max_grad_norm=max_norm)
    weights, stats = _train(g, G, D, 2)
    for name, s in stats[0].items():
        assert s["clip_coef"] < 1.0 and s["skipped"] == 0, (name, s)
        assert abs(s["grad_norm"] - base["on_stats"][0][name]["grad_norm"]) <= 1e-12 * s["grad_norm"], "chunk 1 saw (a)'s gradients"
    for name in weights[0]:
        assert not torch.equal(weights[0][name], base["on"][0][name]), name
        assert torch.isfinite(weights[1][name]).all()
    G.save("latest"); D.save("latest")
    for f in ("latest_net_G0.pth", "latest_net_G1.pth", "latest_net_D.pth", "latest_net_D_T0.pth"):
        assert os.path.isfile(os.path.join(ck, "guard", f)), f


def test_model_skips_a_poisoned_generator_step_and_saves_clean_weights(golden, tmp_path):
    """(c) ema_decay on; a NaN written into optimizer_G's flat gradient between backward and step of chunk 1: that step is
    skipped, for G only, and what save() writes -- raw weights and the averaged ones -- is finite."""
    base = _baseline(golden, tmp_path)
    g, ck = base["g"], str(tmp_path)
    _, G, D = _train_models(g, ck, ema_decay=0.9, skip_nonfinite_grads=True)

    def poison(chunk):
        if chunk == 0:
            fg = G.optimizer_G.flat.flat_grad
            fg[fg.numel() // 2] = float("nan")

    w0, e0 = G.optimizer_G.flat.flat_param.clone(), G.optimizer_G.ema.clone()
    weights, stats = _train(g, G, D, 2, before_G_step=poison)
    assert torch.equal(weights[0]["optimizer_G"], w0), "the poisoned step moved no weight"
    s0, s1 = stats[0]["optimizer_G"], stats[1]["optimizer_G"]
    assert s0["skipped"] == 1 and s0["applied"] == 0 and s0["nonfinite"] >= 1
    assert s1["skipped"] == 1 and s1["applied"] == 1 and s1["nonfinite"] == 0
    assert torch.isfinite(G.optimizer_G.ema).all() and not torch.equal(G.optimizer_G.ema, e0)
    for name in ("optimizer_D", "optimizer_D_T0"):
        assert stats[1][name]["skipped"] == 0 and stats[1][name]["applied"] == 2, name
    assert not torch.equal(weights[0]["optimizer_G"], weights[1]["optimizer_G"]), "the clean chunk trained"
    G.save("latest")
    for s in range(2):
        for suffix in ("", "_ema"):
            sd = torch.load(os.path.join(ck, "guard", "latest_net_G%d%s.pth" % (s, suffix)))
            assert sd and all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point()), (s, suffix)
