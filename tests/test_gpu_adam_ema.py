"""Generator weight averaging fused into the Adam step on the GPU: v2v_adam_step_ema / v2v_adam_step_dev_ema
against the plain entry points (bit contracts), against an fp64 recursion, captured into a graph, and through the model
(training with opt.ema_decay, save(), inference with opt.use_ema)."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from util import sd_from_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
PAD = 8                                   # guard floats in front of and behind every buffer
HYPER = dict(lr=2e-4, b1=0.5, b2=0.999, eps=1e-8)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Bufs:
    """param, grad, exp_avg, exp_avg_sq (>= 0), ema: O(1) seeded normals, each a window of n floats inside an allocation with
    guard floats around it.  offs: the window's start in floats per buffer (4 = 16-byte aligned, torch's allocations are)."""
    names = ("p", "g", "m", "v", "e")

    def __init__(self, n, seed, offs=(4, 4, 4, 4, 4), like=None):
        self.n, self.offs = n, offs
        if like is None:
            gen = torch.Generator(device=DEV).manual_seed(seed)
            vals = [torch.randn(n, device=DEV, generator=gen) for _ in range(5)]
            vals[3] = vals[3] * vals[3]
        else:
            vals = [like.win(k).clone() for k in self.names]
        self.full = {}
        for k, o, val in zip(self.names, offs, vals):
            t = torch.full((n + 2 * PAD,), 12345.0, device=DEV)
            t[o:o + n] = val
            self.full[k] = t

    def win(self, k):
        o = self.offs[self.names.index(k)]
        return self.full[k][o:o + self.n]

    def guards_intact(self):
        for k, o in zip(self.names, self.offs):
            t = self.full[k]
            if not (bool((t[:o] == 12345.0).all()) and bool((t[o + self.n:] == 12345.0).all())):
                return False
        return True


def _host(b, step, wd=0.0, gs=1.0, decay=None):
    from vid2vid_amd.lib import lib, check
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = HYPER
    if decay is None:
        check(lib.v2v_adam_step(_ptr(b.win("p")), _ptr(b.win("g")), _ptr(b.win("m")), _ptr(b.win("v")), b.n,
                                h["lr"], h["b1"], h["b2"], h["eps"], wd, gs, step, s), "adam_step")
    else:
        check(lib.v2v_adam_step_ema(_ptr(b.win("p")), _ptr(b.win("g")), _ptr(b.win("m")), _ptr(b.win("v")), _ptr(b.win("e")), b.n,
                                    h["lr"], h["b1"], h["b2"], h["eps"], wd, gs, step, decay, s), "adam_step_ema")


def _state(step=0):
    host = torch.zeros(2, dtype=torch.int32)
    host[0] = step
    host[1:2].view(torch.float32)[0] = HYPER["lr"]
    return host.to(DEV)


def _dev(b, state, wd=0.0, gs=1.0, decay=None):
    from vid2vid_amd.lib import lib, check
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = HYPER
    if decay is None:
        check(lib.v2v_adam_step_dev(_ptr(b.win("p")), _ptr(b.win("g")), _ptr(b.win("m")), _ptr(b.win("v")), b.n,
                                    h["b1"], h["b2"], h["eps"], wd, gs, _ptr(state), s), "adam_step_dev")
    else:
        check(lib.v2v_adam_step_dev_ema(_ptr(b.win("p")), _ptr(b.win("g")), _ptr(b.win("m")), _ptr(b.win("v")), _ptr(b.win("e")), b.n,
                                        h["b1"], h["b2"], h["eps"], wd, gs, _ptr(state), decay, s), "adam_step_dev_ema")


def _same_adam_state(a, b):
    return all(torch.equal(a.win(k), b.win(k)) for k in ("p", "m", "v"))


SIZES = [1, 255, 1027, 5000, 8192 * 1024 + 3]      # 1027 / 5000: vector tail and grid-stride loop; the last crosses the 8192-block cap


@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (0.01, 1.0), (0.0, 0.5), (0.01, 0.5)])
@pytest.mark.parametrize("n", SIZES)
def test_contract_a_adam_state_is_bit_identical_to_the_plain_step(n, wd, gs):
    """(a): param, exp_avg, exp_avg_sq after the _ema entry points == after the plain ones, host-step form (one call) and
    device-state form (three consecutive calls, the step word included).  The shadow moved and nothing outside [0, n) did."""
    old = Bufs(n, seed=n)
    new = Bufs(n, seed=n, like=old)
    e0, p0 = new.win("e").clone(), new.win("p").clone()
    _host(old, 3, wd, gs); _host(new, 3, wd, gs, decay=0.9)
    assert _same_adam_state(old, new), "host-step form"
    assert not torch.equal(new.win("p"), p0), "the step did run"
    assert not torch.equal(new.win("e"), e0) and torch.equal(old.win("e"), e0)
    so, sn = _state(1), _state(1)
    for it in range(3):
        _dev(old, so, wd, gs); _dev(new, sn, wd, gs, decay=0.9)
        assert _same_adam_state(old, new), "device-state form, call %d" % it
    assert torch.equal(so, sn) and int(sn[0]) == 4
    assert old.guards_intact() and new.guards_intact()
    assert torch.isfinite(new.win("e")).all()


@pytest.mark.parametrize("n", [1, 1027, 5000])
def test_contracts_b_and_c_decay_zero_copies_and_decay_one_keeps(n):
    for form in ("host", "dev"):
        for decay in (0.0, 1.0):
            b = Bufs(n, seed=7 * n)
            e0, p0 = b.win("e").clone(), b.win("p").clone()
            if form == "host":
                _host(b, 2, 0.01, 0.5, decay=decay)
            else:
                _dev(b, _state(1), 0.01, 0.5, decay=decay)
            assert not torch.equal(b.win("p"), p0)
            if decay == 0.0:
                assert torch.equal(b.win("e"), b.win("p")), "(b) %s form: ema == param" % form
            else:
                assert torch.equal(b.win("e"), e0), "(c) %s form: ema untouched" % form
            assert b.guards_intact()


@pytest.mark.parametrize("n", [1, 255, 1027, 5000])
@pytest.mark.parametrize("offs", [(5, 5, 5, 5, 5), (4, 4, 4, 4, 5), (7, 7, 7, 7, 7), (4, 6, 4, 4, 4)],
                         ids=["all+1", "ema+1", "all+3", "grad+2"])
def test_misaligned_buffers_give_the_aligned_bits(n, offs):
    """All five buffers one float off 16 bytes (scalar head, vectors, tail), only `ema` off (no common alignment: scalar
    throughout): every element gets the bits of the aligned run, and the plain step's bits in param / moments."""
    ref = Bufs(n, seed=3 * n + 1)
    mis = Bufs(n, seed=0, offs=offs, like=ref)
    plain = Bufs(n, seed=0, offs=offs, like=ref)
    for k, o in zip(Bufs.names, offs):
        assert (mis.win(k).data_ptr() % 16) == (4 * o) % 16
    _host(ref, 2, 0.01, 0.5, decay=0.9); _host(mis, 2, 0.01, 0.5, decay=0.9); _host(plain, 2, 0.01, 0.5)
    assert all(torch.equal(ref.win(k), mis.win(k)) for k in Bufs.names), "host-step form"
    assert _same_adam_state(plain, mis)
    sr, sm, sp = _state(1), _state(1), _state(1)
    _dev(ref, sr, 0.01, 0.5, decay=0.9); _dev(mis, sm, 0.01, 0.5, decay=0.9); _dev(plain, sp, 0.01, 0.5)
    assert all(torch.equal(ref.win(k), mis.win(k)) for k in Bufs.names), "device-state form"
    assert _same_adam_state(plain, mis)
    assert mis.guards_intact() and ref.guards_intact()


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("decay", [0.5, 0.9])
@pytest.mark.parametrize("n", [1027, 5000])
def test_shadow_against_fp64_recursion(n, decay, form):
    """N = 5 steps; reference: ema <- d * ema + (1 - d) * param in fp64 on the GPU's own fp32 weights after each step, d the
    fp32 value the kernel was handed.  Per step the kernel rounds (1 - d) * param and the fma, and (1 - d) itself was rounded
    once: each at most 2^-24 relative to a value no larger than max(|ema|, |param|); the recursion multiplies earlier error
    by d < 1.  Bound, per element: 3 * N * 2^-24 * max(|ema|, |param|)."""
    N = 5
    b = Bufs(n, seed=11 * n)
    d = float(torch.tensor(decay, dtype=torch.float32))
    ref = b.win("e").double()
    state = _state(0)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for it in range(N):
        b.win("g").copy_(torch.randn(n, device=DEV, generator=gen))
        if form == "host":
            _host(b, it + 1, 0.01, 1.0, decay=decay)
        else:
            _dev(b, state, 0.01, 1.0, decay=decay)
        ref = d * ref + (1.0 - d) * b.win("p").double()
    err = (b.win("e").double() - ref).abs()
    bound = 3 * N * 2.0 ** -24 * torch.maximum(b.win("e").abs(), b.win("p").abs()).double()
    print("n=%d decay=%g %s: max err %.3e, max err/bound %.3f" % (n, decay, form, err.max().item(), (err / bound).max().item()))
    assert bool((err <= bound).all())
    assert b.guards_intact()


def _twin_optimizers(ema_decay, capturable):
    from vid2vid_amd.optim import FusedAdam
    torch.manual_seed(41)
    shapes = [(7, 5, 3, 3), (13,), (4, 9)]
    base = [torch.randn(*s) for s in shapes]
    out = []
    for _ in range(2):
        ps = [nn.Parameter(t.clone().to(DEV)) for t in base]
        opt = FusedAdam(ps, lr=2e-4, betas=(0.5, 0.999), ema_decay=ema_decay)
        if capturable:
            opt.make_capturable()
        out.append(opt)
    return out


def test_capturable_step_with_shadow_replays_in_a_graph():
    """optimizer.step() of a capturable FusedAdam(ema_decay) captured once with torch.cuda.graph: three replays == three eager
    steps (weights, moments, shadow and the device step count, bit for bit)."""
    graphed, eager = _twin_optimizers(0.9, True)
    plain, warm = _twin_optimizers(None, True)
    warm.step(); _twin_optimizers(0.9, True)[0].step()     # both kernels have run once before anything is captured
    gen = torch.Generator(device=DEV).manual_seed(9)
    grads = [torch.randn(graphed.flat.numel, device=DEV, generator=gen) for _ in range(3)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    keep = {k: getattr(graphed, k).clone() for k in ("exp_avg", "exp_avg_sq", "ema")}
    keep["p"] = graphed.flat.flat_param.clone()
    with torch.cuda.graph(g):
        graphed.step()
    assert graphed.device_step() == 0 and torch.equal(graphed.ema, keep["ema"]), "capture launches nothing"
    for gr in grads:
        graphed.flat.flat_grad.copy_(gr); g.replay()
        eager.flat.flat_grad.copy_(gr); eager.step()
        plain.flat.flat_grad.copy_(gr); plain.step()
    torch.cuda.synchronize()
    assert graphed.device_step() == 3 and eager.device_step() == 3
    assert torch.equal(graphed.flat.flat_param, eager.flat.flat_param) and not torch.equal(graphed.flat.flat_param, keep["p"])
    assert torch.equal(graphed.exp_avg, eager.exp_avg) and torch.equal(graphed.exp_avg_sq, eager.exp_avg_sq)
    assert torch.equal(graphed.ema, eager.ema) and not torch.equal(graphed.ema, keep["ema"])
    assert torch.equal(graphed.flat.flat_param, plain.flat.flat_param), "and the weights of an optimizer without a shadow"


def test_overlapped_step_updates_the_shadow_on_the_side_stream():
    """GradSync.run_overlapped (a world-size-1 RCCL group with the collective forced on): the _ema kernel runs on the side
    stream like the moments' update; after wait_pending the shadow equals an un-synchronised optimizer's."""
    import os, socket
    import torch.distributed as dist
    from vid2vid_amd import parallel
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        oa, ob = _twin_optimizers(0.9, False)
        gs = parallel.sync_optimizers([oa], bucket_bytes=1 << 10, force_collective=True)
        gen = torch.Generator(device=DEV).manual_seed(10)
        for it in range(3):
            gr = torch.randn(oa.flat.numel, device=DEV, generator=gen)
            oa.zero_grad(); ob.zero_grad()
            oa.flat.flat_grad.copy_(gr); ob.flat.flat_grad.copy_(gr)
            oa.step(); ob.step()
            assert gs.pending(oa)
        sd = oa.ema_state_dict(nn.ParameterList(oa.flat.params))            # waits for the pending step by itself
        assert not gs.pending(oa)
        torch.cuda.synchronize()
        assert torch.equal(oa.flat.flat_param, ob.flat.flat_param) and torch.equal(oa.ema, ob.ema)
        assert not torch.equal(oa.ema, oa.flat.flat_param)
        for (k, v), w in zip(sd.items(), ob.ema_views().values()):
            assert torch.equal(v, w.cpu()), k
    finally:
        parallel._ACTIVE_SYNCS.clear()
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------- model level
def _train_models(g, ckpt, ema_decay):
    """The golden training configuration (tests/golden/training_label2city_s2_32x64.npz's shapes and weights)."""
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models.vid2vid_model_G import Vid2VidModelG
    from vid2vid_amd.models.vid2vid_model_D import Vid2VidModelD
    opt = make_opt(isTrain=True, label_nc=35, loadSize=64, use_instance=True, fg=True, ngf=8, n_blocks=2,
                   n_blocks_local=1, n_scales_spatial=2, n_downsample_G=2, no_vgg=True, num_D=2, ndf=8,
                   n_frames_total=6, max_frames_per_gpu=3, n_scales_temporal=1, niter_fix_global=0,
                   precision="fp32", gpu_ids=[0], random_init_ok=True, ema_decay=ema_decay,
                   checkpoints_dir=ckpt, name="ema")
    G = Vid2VidModelG(); G.initialize(opt)
    D = Vid2VidModelD(); D.initialize(opt)
    G.netG0.load_state_dict(sd_from_npz(g, "sdG0."))
    G.netG1.load_state_dict(sd_from_npz(g, "sdG1."))
    D.netD.load_state_dict(sd_from_npz(g, "sdD."))
    D.netD_T0.load_state_dict(sd_from_npz(g, "sdDT0."))
    if ema_decay:
        G.optimizer_G.seed_ema()                          # the weights were replaced behind the optimizer's back
    return opt, G, D


def _train(g, G, D, n_chunks):
    """train.py:50-95 per chunk with the fixture's flow_ref / conf_ref standing in for FlowNet2; returns the generator's flat
    weights after every chunk (first entry: before training)."""
    lab, inst, Bimg = T(g["in.labels"]).to(DEV), T(g["in.inst"]).to(DEV), T(g["in.B"]).to(DEV)
    flow_ref, conf_ref = T(g["in.flow_ref"]).to(DEV), T(g["in.conf_ref"]).to(DEV)
    reshape = lambda ts: [None if t is None else t.contiguous().view(-1, t.size(2), t.size(3), t.size(4)) for t in ts]
    weights = [G.optimizer_G.flat.flat_param.clone()]
    for _ in range(n_chunks):
        fake_B, fake_B_raw, flow, weight, real_A, real_Bp, fake_B_last = G(lab, Bimg, inst, None)
        real_B_prev, real_B = real_Bp[:, :-1], real_Bp[:, 1:]
        fake_B_prev = G.compute_fake_B_prev(real_B_prev, None, fake_B)
        losses = D(0, reshape([real_B, fake_B, fake_B_raw, real_A, real_B_prev, fake_B_prev, flow, weight, flow_ref, conf_ref]))
        loss_dict = dict(zip(D.loss_names, [torch.mean(x) for x in losses]))
        _, skipped = D.get_all_skipped_frames((None,) * 4, real_B, fake_B, flow_ref, conf_ref, 1, 3, G.n_frames_load, 0, None)
        lt = D(1, [f[0] for f in skipped])
        loss_dict_T = [dict(zip(D.loss_names_T, [torch.mean(x) for x in lt]))]
        loss_G, loss_D, loss_D_T, _ = D.get_losses(loss_dict, loss_dict_T, 1)
        G.optimizer_G.zero_grad(); loss_G.backward(); G.optimizer_G.step()
        D.optimizer_D.zero_grad(); loss_D.backward(); D.optimizer_D.step()
        D.optimizer_D_T0.zero_grad(); loss_D_T[0].backward(); D.optimizer_D_T0.step()
        torch.cuda.synchronize()
        weights.append(G.optimizer_G.flat.flat_param.clone())
    return weights


def _infer(model, H=32, W=64):
    from vid2vid_amd import synthetic
    lab, inst, frames = synthetic.label2city_sequence(4, H, W, seed=7)
    model.fake_B_prev = None
    outs = []
    for t in range(2):
        fake, _ = model.inference(lab[t:t + 3].view(1, 3, 1, H, W), frames[:, :2] if t == 0 else None,
                                  inst[t:t + 3].view(1, 3, 1, H, W))
        outs.append(fake.float().clone())
    return torch.cat(outs)


def test_model_trains_saves_and_serves_the_shadow(golden, tmp_path):
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    g = golden("training_label2city_s2_32x64")
    ck = str(tmp_path)
    decay, n_chunks = 0.9, 3
    # tile cache: a throw-away chunk lets the engine pick (and keep) a tile for every shape of this configuration; the two
    # compared runs below then replay the same selections
    opt, G, D = _train_models(g, ck, 0.0)
    _train(g, G, D, 1)
    eng = G.engine
    pinned = dict(eng._tuned)

    opt, G, D = _train_models(g, ck, 0.0)
    assert not hasattr(G.optimizer_G, "ema")
    w_off = _train(g, G, D, n_chunks)
    opt, G, D = _train_models(g, ck, decay)
    w_on = _train(g, G, D, n_chunks)
    assert dict(eng._tuned) == pinned, "a tile was searched between the compared runs"
    for k, (a, b) in enumerate(zip(w_off, w_on)):
        assert torch.equal(a, b), "weights after chunk %d differ from the run without ema_decay" % k
    assert not torch.equal(w_on[0], w_on[-1])

    # the shadow against the fp64 recursion over the recorded weights (bound: test_shadow_against_fp64_recursion)
    live = G.optimizer_G
    d = float(torch.tensor(decay, dtype=torch.float32))
    ref = w_on[0].double()
    for w in w_on[1:]:
        ref = d * ref + (1.0 - d) * w.double()
    err = (live.ema.double() - ref).abs()
    bound = 3 * n_chunks * 2.0 ** -24 * torch.maximum(live.ema.abs(), w_on[-1].abs()).double()
    print("model shadow: max err %.3e, max err/bound %.3f" % (err.max().item(), (err / bound.clamp_min(1e-300)).max().item()))
    assert bool((err <= bound).all())
    assert not torch.equal(live.ema, w_on[-1]) and not torch.equal(live.ema, w_on[0])

    # save(), then inference with opt.use_ema against a plain model into which the shadow is copied by hand
    G.save("latest")
    kw = dict(name="ema", checkpoints_dir=ck, label_nc=35, use_instance=True, fg=True, use_real_img=True, ngf=8, n_blocks=2,
              n_blocks_local=1, n_scales_spatial=2, n_downsample_G=2, loadSize=64, precision="fp32", gpu_ids=[0])
    served = create_model(make_opt(use_ema=True, **kw))
    plain = create_model(make_opt(**kw))
    views = live.ema_views()
    with torch.no_grad():
        for s in range(2):
            src = dict(getattr(G, "netG%d" % s).named_parameters())
            for name, p in getattr(plain, "netG%d" % s).named_parameters():
                assert torch.equal(p.detach(), src[name].detach()), name          # save() wrote the raw weights as ever
                p.copy_(views[src[name]])
    plain.engine.refresh_weights()
    by_hand = _infer(plain)
    got = _infer(served)
    assert torch.isfinite(got).all()
    assert torch.equal(got, by_hand)
