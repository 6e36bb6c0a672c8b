"""Generator weight averaging without a GPU: the argument checks of v2v_adam_step_ema / v2v_adam_step_dev_ema
in the library's dry-run mode, FusedAdam(ema_decay=...)'s bookkeeping (state_dict round trip, re-seeding, rebuild carry-over,
ema_state_dict), and what Vid2VidModelG.save() writes.  Nothing here executes a kernel: values only move through torch copies."""
import ctypes as C
import os

import pytest
import torch
import torch.nn as nn

from vid2vid_amd import lib as L
from vid2vid_amd import networks as N

EINVAL = -1          # V2V_EINVAL (include/v2v_hip.h)


@pytest.fixture()
def dry_run():
    N.set_record_only(True)
    yield
    N.set_record_only(False)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _host(p, g, m, v, e, n, decay, step=1):
    return L.lib.v2v_adam_step_ema(p, g, m, v, e, n, 2e-4, 0.5, 0.999, 1e-8, 0.0, 1.0, step, decay, None)


def _dev(p, g, m, v, e, n, decay, state):
    return L.lib.v2v_adam_step_dev_ema(p, g, m, v, e, n, 0.5, 0.999, 1e-8, 0.0, 1.0, state, decay, None)


def test_entry_points_refuse_bad_arguments(dry_run):
    n = 64
    big = torch.zeros(6 * n)
    p, g, m, v, e = (big[i * n:(i + 1) * n] for i in range(5))
    state = torch.zeros(2, dtype=torch.int32)
    calls = {"host": lambda *a: _host(*a), "dev": lambda *a: _dev(*a, _ptr(state))}
    for name, call in calls.items():
        ok = (_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e), n)
        assert call(*ok, 0.9) == 0, name                                        # (ema starts where exp_avg_sq ends: adjacent is fine)
        assert call(*ok, 0.0) == 0 and call(*ok, 1.0) == 0, name               # the closed interval
        assert call(*ok[:4], None, n, 0.9) == EINVAL, name                    # null ema
        for bad in (-0.1, 1.5, float("nan"), float("inf")):
            assert call(*ok, bad) == EINVAL, (name, bad)
        for k in range(4):                                                      # ema overlapping each of the other four
            assert call(*ok[:4], _ptr((p, g, m, v)[k]), n, 0.9) == EINVAL, (name, k)
            assert call(*ok[:4], _ptr((p, g, m, v)[k][n - 1:]), n, 0.9) == EINVAL, (name, k)     # by one element
        # what the plain entry points refuse
        for k in range(4):
            a = list(ok); a[k] = None
            assert call(*a, 0.9) == EINVAL, (name, k)
        assert call(*ok[:5], 0, 0.9) == EINVAL, name
    assert _host(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e), n, 0.9, step=0) == EINVAL
    assert _dev(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e), n, 0.9, None) == EINVAL


def _params(seed=0, shapes=((4, 3, 3, 3), (7,), (5, 6))):
    gen = torch.Generator().manual_seed(seed)
    return [nn.Parameter(torch.randn(*s, generator=gen)) for s in shapes]


def test_off_optimizer_is_what_it_was(dry_run):
    from vid2vid_amd.optim import FusedAdam
    keys = {"step", "exp_avg", "exp_avg_sq", "numel", "hyper"}
    for off in (None, 0, 0.0):
        opt = FusedAdam(_params(), ema_decay=off)
        assert not hasattr(opt, "ema")
        assert set(opt.state_dict()) == keys
        opt.zero_grad(); opt.step()                       # the plain entry point, argument-checked by the library
        with pytest.raises(RuntimeError):
            opt.ema_views()
    assert set(FusedAdam(_params()).state_dict()) == keys
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            FusedAdam(_params(), ema_decay=bad)


def test_on_optimizer_steps_through_the_ema_entry_points(dry_run):
    from vid2vid_amd.optim import FusedAdam
    ps = _params()
    opt = FusedAdam(ps, ema_decay=0.9)
    assert opt.ema.dtype == torch.float32 and opt.ema.shape == opt.flat.flat_param.shape
    assert torch.equal(opt.ema, opt.flat.flat_param) and opt.ema.data_ptr() != opt.flat.flat_param.data_ptr()
    views = opt.ema_views()
    assert list(views) == opt.flat.params
    for p, o in zip(opt.flat.params, opt.flat.offsets):
        assert views[p].shape == p.shape and views[p].data_ptr() == opt.ema.data_ptr() + 4 * o
        assert torch.equal(views[p], p.detach())
    opt.zero_grad(); opt.step()
    opt.make_capturable()
    opt.zero_grad(); opt.step()
    assert opt.step_count == 2


def test_state_dict_round_trip_and_reseeding(dry_run):
    from vid2vid_amd.optim import FusedAdam
    a = FusedAdam(_params(1), ema_decay=0.75)
    with torch.no_grad():
        a.ema.copy_(torch.arange(a.flat.numel, dtype=torch.float32))
        a.exp_avg.fill_(0.25)
    sd = a.state_dict()
    assert set(sd) == {"step", "exp_avg", "exp_avg_sq", "numel", "hyper", "ema", "ema_decay"}
    assert sd["ema_decay"] == 0.75 and sd["ema"].device.type == "cpu" and torch.equal(sd["ema"], a.ema)
    assert sd["ema"].data_ptr() != a.ema.data_ptr()
    b = FusedAdam(_params(2), ema_decay=0.9)
    b.load_state_dict(sd)
    assert torch.equal(b.ema, a.ema) and b.ema_decay == 0.75 and torch.equal(b.exp_avg, a.exp_avg)
    # a checkpoint of a run without averaging: the shadow restarts from the current weights
    old = {k: v for k, v in sd.items() if k not in ("ema", "ema_decay")}
    c = FusedAdam(_params(3), ema_decay=0.9)
    with torch.no_grad():
        c.ema.zero_()
    c.load_state_dict(old)
    assert torch.equal(c.ema, c.flat.flat_param) and c.ema_decay == 0.9
    # an optimizer without averaging loads a checkpoint that has it and stays as it is
    d = FusedAdam(_params(4))
    d.load_state_dict(sd)
    assert not hasattr(d, "ema") and "ema" not in d.state_dict()


def test_rebuild_keeps_tracked_shadows_and_seeds_new_parameters(dry_run):
    from vid2vid_amd.optim import FusedAdam
    old = _params(5)
    opt = FusedAdam(old, ema_decay=0.9)
    with torch.no_grad():
        for i, v in enumerate(opt.ema_views().values()):
            v.fill_(10.0 + i)
    new = _params(6, shapes=((3, 2), (9,)))
    weights = [p.detach().clone() for p in new + old]
    opt.rebuild(new + old)                                # new parameters FIRST: every offset moves
    views = opt.ema_views()
    assert list(views) == new + old and opt.ema.numel() == opt.flat.numel
    for i, p in enumerate(old):
        assert torch.equal(views[p], torch.full(p.shape, 10.0 + i)), "carried over by parameter identity"
    for p in new:
        assert torch.equal(views[p], p.detach()), "seeded from the current weights"
    for p, w in zip(new + old, weights):
        assert torch.equal(p.detach(), w)
    opt.zero_grad(); opt.step()


def test_ema_state_dict_has_the_networks_keys(dry_run):
    from vid2vid_amd.optim import FusedAdam
    net = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Conv2d(4, 2, 1))
    for p in net[2].parameters():
        p.requires_grad_(False)                           # not tracked: passes through
    opt = FusedAdam([p for p in net.parameters() if p.requires_grad], ema_decay=0.9)
    with torch.no_grad():
        opt.ema.fill_(7.0)
        net[1].running_mean.fill_(3.0)
    sd = opt.ema_state_dict(net)
    ref = net.state_dict()
    assert list(sd) == list(ref)
    tracked = {k for k, p in net.named_parameters() if p.requires_grad}
    for k, v in sd.items():
        assert v.device.type == "cpu" and v.is_contiguous() and v.shape == ref[k].shape and v.dtype == ref[k].dtype
        if k in tracked:
            assert torch.equal(v, torch.full(v.shape, 7.0)), k
        else:
            assert torch.equal(v, ref[k]), k
    assert torch.equal(sd["1.running_mean"], torch.full((4,), 3.0)) and "1.num_batches_tracked" in sd


def _train_opt(tmp_path, **kw):
    from vid2vid_amd.options import make_opt
    d = dict(isTrain=True, label_nc=35, use_instance=True, fg=True, ngf=8, n_blocks=2, n_blocks_local=1, n_scales_spatial=2,
             n_downsample_G=2, loadSize=64, no_vgg=True, random_init_ok=True, precision="fp32", gpu_ids=[], n_gpus_gen=1,
             checkpoints_dir=str(tmp_path), name="ema")
    d.update(kw)
    return make_opt(**d)


def test_make_opt_accepts_the_two_options():
    from vid2vid_amd.options import make_opt
    opt = make_opt()
    assert opt.ema_decay == 0.0 and opt.use_ema is False
    opt = make_opt(ema_decay=0.999, use_ema=True)
    assert opt.ema_decay == 0.999 and opt.use_ema is True


def test_save_writes_the_shadow_only_when_enabled(dry_run, tmp_path):
    from vid2vid_amd.models.vid2vid_model_G import Vid2VidModelG
    from vid2vid_amd.models.base_model import _UnsteppedAdam
    ck = os.path.join(str(tmp_path), "ema")
    listing = lambda: sorted(f for f in os.listdir(ck) if f.endswith(".pth"))

    G = Vid2VidModelG(); G.initialize(_train_opt(tmp_path))
    assert not hasattr(G.optimizer_G, "ema")
    G.save("off")
    assert listing() == ["off_net_G0.pth", "off_net_G1.pth"]

    # every scale trained: a shadow file per scale, with save_network's key set
    G = Vid2VidModelG(); G.initialize(_train_opt(tmp_path, ema_decay=0.9, niter_fix_global=0))
    assert G.optimizer_G.ema_decay == 0.9
    with torch.no_grad():
        G.optimizer_G.ema.fill_(0.5)
    G.save("all")
    assert [f for f in listing() if f.startswith("all")] == ["all_net_G0.pth", "all_net_G0_ema.pth", "all_net_G1.pth", "all_net_G1_ema.pth"]
    for s in range(2):
        raw = torch.load(os.path.join(ck, "all_net_G%d.pth" % s))
        ema = torch.load(os.path.join(ck, "all_net_G%d_ema.pth" % s))
        assert list(ema) == list(raw)
        names = {k for k, _ in getattr(G, "netG%d" % s).named_parameters()}
        for k in raw:
            if k in names:
                assert torch.equal(ema[k], torch.full(raw[k].shape, 0.5)), k
            else:
                assert torch.equal(ema[k], raw[k]), k

    # finest scale only, then the reference-compatible update_fixed_params: optimizer_G becomes an unstepped stand-in and the
    # shadow lives on in the optimizer train.py keeps stepping
    G = Vid2VidModelG(); G.initialize(_train_opt(tmp_path, ema_decay=0.9, niter_fix_global=1))
    G.save("fine")
    assert [f for f in listing() if f.startswith("fine")] == ["fine_net_G0.pth", "fine_net_G1.pth", "fine_net_G1_ema.pth"]
    live = G.optimizer_G
    G.update_fixed_params()
    assert isinstance(G.optimizer_G, _UnsteppedAdam) and G._optimizer_G_live is live
    with torch.no_grad():
        live.ema.fill_(0.25)
    G.save("late")
    assert [f for f in listing() if f.startswith("late")] == ["late_net_G0.pth", "late_net_G1.pth", "late_net_G1_ema.pth"]
    w = torch.load(os.path.join(ck, "late_net_G1_ema.pth"))
    name = next(k for k, _ in G.netG1.named_parameters())
    assert torch.equal(w[name], torch.full(w[name].shape, 0.25))


def test_continue_train_seeds_the_shadow_from_the_ema_file(dry_run, tmp_path):
    from vid2vid_amd.models.vid2vid_model_G import Vid2VidModelG
    G = Vid2VidModelG(); G.initialize(_train_opt(tmp_path, ema_decay=0.9))
    with torch.no_grad():
        G.optimizer_G.ema.fill_(0.125)
    G.save("latest")
    os.remove(os.path.join(str(tmp_path), "ema", "latest_net_G0_ema.pth"))          # scale 0 has no shadow file
    R = Vid2VidModelG(); R.initialize(_train_opt(tmp_path, ema_decay=0.9, continue_train=True))
    views = R.optimizer_G.ema_views()
    for p in R.netG1.parameters():
        assert torch.equal(views[p], torch.full(p.shape, 0.125)), "from latest_net_G1_ema.pth"
    for (k, p), q in zip(R.netG0.named_parameters(), G.netG0.parameters()):
        assert torch.equal(p.detach(), q.detach()), k
        assert torch.equal(views[p], p.detach()), "no file: the loaded weights"


def test_use_ema_loads_the_shadow_file(dry_run, tmp_path):
    from vid2vid_amd.models.vid2vid_model_G import Vid2VidModelG
    G = Vid2VidModelG(); G.initialize(_train_opt(tmp_path, ema_decay=0.9))
    with torch.no_grad():
        G.optimizer_G.ema.fill_(0.375)
    G.save("latest")
    kw = dict(isTrain=False, random_init_ok=False, use_real_img=True)
    M = Vid2VidModelG(); M.initialize(_train_opt(tmp_path, use_ema=True, **kw))
    P = Vid2VidModelG(); P.initialize(_train_opt(tmp_path, **kw))
    for s in range(2):
        for (k, p), q, r in zip(getattr(M, "netG%d" % s).named_parameters(), getattr(P, "netG%d" % s).parameters(),
                                getattr(G, "netG%d" % s).parameters()):
            assert torch.equal(p.detach(), torch.full(p.shape, 0.375)), k
            assert torch.equal(q.detach(), r.detach()), k
    os.remove(os.path.join(str(tmp_path), "ema", "latest_net_G0_ema.pth"))
    with pytest.raises(RuntimeError, match="Generator must exist"):
        Vid2VidModelG().initialize(_train_opt(tmp_path, use_ema=True, **kw))
    Vid2VidModelG().initialize(_train_opt(tmp_path, use_ema=True, **dict(kw, random_init_ok=True)))
