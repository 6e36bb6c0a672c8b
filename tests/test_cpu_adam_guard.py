"""The gradient guard of the fused Adam step without a GPU: what a step records in the library's dry-run mode with
the options off (the parent's ops, nothing else) and on (sum of squares -> finalize -> guarded update), the argument checks of
the new entry points, FusedAdam's bookkeeping (state_dict, rebuild) and the options' way into every training optimizer.
Nothing here executes a kernel."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
from vid2vid_amd import lib as L
from vid2vid_amd import networks as N

EINVAL = -1          # V2V_EINVAL (include/v2v_hip.h)
NEW = ("v2v_adam_guard_workspace_bytes", "v2v_grad_sumsq", "v2v_adam_step_dev_guard", "v2v_adam_step_dev_guard_ema")


@pytest.fixture()
def dry_run():
    N.set_record_only(True)
    yield
    N.set_record_only(False)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _params(seed=0, shapes=((4, 3, 3, 3), (7,), (5, 6))):
    gen = torch.Generator().manual_seed(seed)
    return [nn.Parameter(torch.randn(*s, generator=gen)) for s in shapes]


def _recorded(fn):
    lib = L.lib
    plan = lib.v2v_plan_create()
    try:
        assert lib.v2v_plan_begin_record(plan) == 0
        try:
            fn()
        finally:
            assert lib.v2v_plan_end_record(plan) == 0
        return [lib.v2v_plan_op_name(plan, i).decode() for i in range(lib.v2v_plan_num_ops(plan))]
    finally:
        lib.v2v_plan_destroy(plan)


def test_options_off_a_step_records_what_it_always_did(dry_run):
    """The "nothing changed" pin: passes before and after the guard exists."""
    from vid2vid_amd.optim import FusedAdam
    for ema, host, dev in ((None, "adam_step", "adam_step_dev"), (0.9, "adam_step_ema", "adam_step_dev_ema")):
        opt = FusedAdam(_params(), ema_decay=ema)
        assert not hasattr(opt, "_guard") and not hasattr(opt, "guard") and not opt.capturable
        assert "skipped" not in opt.state_dict()
        assert _recorded(opt.zero_grad) == ["memset_zero"]
        assert _recorded(opt.step) == [host]
        opt.make_capturable()
        assert _recorded(opt.step) == [dev]


@pytest.mark.parametrize("kw", [dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(max_grad_norm=0.5, skip_nonfinite=True)],
                         ids=["clip", "skip", "both"])
def test_either_option_on_records_the_three_launches(dry_run, kw):
    from vid2vid_amd.optim import FusedAdam
    for ema, last in ((None, "adam_step_dev_guard"), (0.9, "adam_step_dev_guard_ema")):
        opt = FusedAdam(_params(), ema_decay=ema, **kw)
        assert opt.capturable and opt.guarded, "a guarded optimizer keeps its step count on the device"
        assert opt._guard.numel() * 4 == L.lib.v2v_adam_guard_workspace_bytes() and not bool(opt._guard.any())
        names = _recorded(opt.step)
        assert names == ["grad_sumsq", "guard_finalize", last]          # (adam_tick is a launch inside the unguarded ops only)
        assert _recorded(opt.zero_grad) == ["memset_zero"]
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            FusedAdam(_params(), max_grad_norm=bad)
    off = FusedAdam(_params(), max_grad_norm=None, skip_nonfinite=False)
    assert not off.guarded and not off.capturable
    with pytest.raises(RuntimeError):
        off.guard_stats()


def test_guard_stats_and_state_dict_round_trip(dry_run):
    from vid2vid_amd.optim import FusedAdam
    a = FusedAdam(_params(1), max_grad_norm=2.0, skip_nonfinite=True)
    assert a.guard_stats() == {"grad_norm": 0.0, "clip_coef": 1.0, "skipped": 0, "applied": 0, "nonfinite": 0}
    a._guard[4] = 3                                        # three steps were skipped (the dry run moves no value by itself)
    a.step_count = 7; a.make_capturable()
    sd = a.state_dict()
    assert set(sd) == {"step", "exp_avg", "exp_avg_sq", "numel", "hyper", "skipped"}
    assert sd["skipped"] == 3 and sd["step"] == 7
    b = FusedAdam(_params(2), skip_nonfinite=True)
    b.load_state_dict(sd)
    assert b.guard_stats()["skipped"] == 3 and b.guard_stats()["applied"] == 7 and b.device_step() == 7
    assert b.state_dict()["skipped"] == 3
    # a checkpoint without the count (an unguarded run, or one from before the guard existed)
    old = {k: v for k, v in sd.items() if k != "skipped"}
    c = FusedAdam(_params(3), max_grad_norm=1.0)
    c._guard[4] = 9
    c.load_state_dict(old)
    assert c.guard_stats()["skipped"] == 0 and c.device_step() == 7
    plain = FusedAdam(_params(4))
    c.load_state_dict(plain.state_dict())
    assert c.device_step() == 0
    # an unguarded optimizer loads a guarded checkpoint and stays as it is
    plain.load_state_dict(sd)
    assert not hasattr(plain, "_guard") and "skipped" not in plain.state_dict() and plain.step_count == 7


def test_rebuild_keeps_the_settings_and_the_skipped_count(dry_run):
    from vid2vid_amd.optim import FusedAdam
    old = _params(5)
    opt = FusedAdam(old, max_grad_norm=0.25, skip_nonfinite=True, ema_decay=0.9)
    opt._guard[4] = 2
    before = opt._guard
    new = _params(6, shapes=((3, 2), (9,)))
    opt.rebuild(new + old)
    assert opt._guard is not before and opt._guard.numel() == before.numel()
    assert opt.max_grad_norm == 0.25 and opt.skip_nonfinite and opt.capturable
    s = opt.guard_stats()
    assert s["skipped"] == 2 and s["applied"] == 0 and opt.device_step() == 0
    assert _recorded(opt.step) == ["grad_sumsq", "guard_finalize", "adam_step_dev_guard_ema"]


def test_entry_points_refuse_bad_arguments(dry_run):
    lib = L.lib
    n = 64
    gbytes = int(lib.v2v_adam_guard_workspace_bytes())
    assert gbytes >= 32 + 1024 * 12 and gbytes % 8 == 0
    big = torch.zeros(5 * n + gbytes // 4 + 4)
    p, g, m, v, e = (big[i * n:(i + 1) * n] for i in range(5))
    guard = big[5 * n:]                                   # starts where `ema` ends: adjacent is fine
    assert guard.data_ptr() % 8 == 0
    state = torch.zeros(2, dtype=torch.int32)
    hyper = (0.5, 0.999, 1e-8, 0.0, 1.0)

    def plain(bufs, n_, st, gd, max_norm=1.0):
        return lib.v2v_adam_step_dev_guard(*bufs[:4], n_, *hyper, st, gd, max_norm, 1, None)

    def ema(bufs, n_, st, gd, max_norm=1.0, decay=0.9):
        return lib.v2v_adam_step_dev_guard_ema(*bufs, n_, *hyper, st, decay, gd, max_norm, 1, None)

    ok = [_ptr(t) for t in (p, g, m, v, e)]
    for name, call, nbuf in (("plain", plain, 4), ("ema", ema, 5)):
        assert call(ok, n, _ptr(state), _ptr(guard)) == 0, name
        for max_norm in (0.0, 1e30, float("inf")):
            assert call(ok, n, _ptr(state), _ptr(guard), max_norm) == 0, (name, max_norm)
        for max_norm in (-1.0, float("nan"), float("-inf")):
            assert call(ok, n, _ptr(state), _ptr(guard), max_norm) == EINVAL, (name, max_norm)
            assert b"max_norm" in lib.v2v_last_error()
        for k in range(nbuf):                              # null pointers
            a = list(ok); a[k] = None
            assert call(a, n, _ptr(state), _ptr(guard)) == EINVAL, (name, k)
        assert call(ok, 0, _ptr(state), _ptr(guard)) == EINVAL and call(ok, -3, _ptr(state), _ptr(guard)) == EINVAL, name
        assert call(ok, n, None, _ptr(guard)) == EINVAL, name
        assert call(ok, n, _ptr(state), None) == EINVAL, name
        assert call(ok, n, _ptr(state), _ptr(guard[1:])) == EINVAL and b"aligned" in lib.v2v_last_error(), name
        for k in range(nbuf):                              # the guard block inside, and one element into, each buffer
            t = (p, g, m, v, e)[k]
            assert call(ok, n, _ptr(state), _ptr(t)) == EINVAL and b"overlaps" in lib.v2v_last_error(), (name, k)
            assert call(ok, n, _ptr(state), _ptr(t[n - 2:])) == EINVAL, (name, k)
        assert call(ok, n, _ptr(guard[2:]), _ptr(guard)) == EINVAL, "the state words inside the guard block"
    for bad in (-0.1, 1.5, float("nan")):                  # what the unguarded _ema entry refuses
        assert ema(ok, n, _ptr(state), _ptr(guard), decay=bad) == EINVAL
    assert ema(ok[:4] + [_ptr(p)], n, _ptr(state), _ptr(guard)) == EINVAL
    # the reduction on its own
    assert lib.v2v_grad_sumsq(_ptr(g), n, _ptr(guard), None) == 0
    assert lib.v2v_grad_sumsq(_ptr(g[1:]), n - 1, _ptr(guard), None) == 0
    assert lib.v2v_grad_sumsq(None, n, _ptr(guard), None) == EINVAL
    assert lib.v2v_grad_sumsq(_ptr(g), 0, _ptr(guard), None) == EINVAL
    assert lib.v2v_grad_sumsq(_ptr(g), n, None, None) == EINVAL
    assert lib.v2v_grad_sumsq(_ptr(g), n, _ptr(guard[1:]), None) == EINVAL
    assert lib.v2v_grad_sumsq(_ptr(g), n, _ptr(g[8:]), None) == EINVAL
    assert _recorded(lambda: lib.v2v_grad_sumsq(_ptr(g), n, _ptr(guard), None)) == ["grad_sumsq", "guard_finalize"]


def _header_args(header, name):
    m = re.search(r"\bint(?:64_t)?\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
    assert m, "%s is not declared in include/v2v_hip.h" % name
    return [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]


def test_header_and_signature_table_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    for name in NEW:
        assert hasattr(L.lib, name), "libv2v_hip.so does not export %s" % name
        assert name in L.exported_symbols()
        args = _header_args(header, name)
        ret, proto = L.PROTOTYPES[name]
        assert len(args) == len(proto), name
        for a, t in zip(args, proto):                      # pointer / integer / float, argument by argument
            want = C.c_void_p if "*" in a else C.c_float if re.match(r"\s*float\b", a) else C.c_int64 if "int64_t" in a else C.c_int32
            assert t is want or (want is C.c_int32 and t is C.c_int), (name, a, t)
    assert L.PROTOTYPES["v2v_adam_guard_workspace_bytes"][0] is C.c_int64
    src = open(os.path.join(ROOT, "vid2vid_amd", "csrc", "train_ops.hip")).read()
    assert "atomicAdd" not in src, "fixed-order reductions only: no floating-point atomics"


def test_make_opt_accepts_the_two_options():
    from vid2vid_amd.options import make_opt
    opt = make_opt()
    assert opt.max_grad_norm == 0.0 and opt.skip_nonfinite_grads is False
    opt = make_opt(max_grad_norm=5.0, skip_nonfinite_grads=True)
    assert opt.max_grad_norm == 5.0 and opt.skip_nonfinite_grads is True


def _train_opt(tmp_path, **kw):
    from vid2vid_amd.options import make_opt
    d = dict(isTrain=True, label_nc=35, use_instance=True, fg=True, ngf=8, ndf=8, num_D=2, n_blocks=2, n_blocks_local=1,
             n_scales_spatial=2, n_scales_temporal=2, n_downsample_G=2, loadSize=64, no_vgg=True, random_init_ok=True,
             precision="fp32", gpu_ids=[], n_gpus_gen=1, checkpoints_dir=str(tmp_path), name="guard")
    d.update(kw)
    return make_opt(**d)


def _models(opt):
    from vid2vid_amd.models.vid2vid_model_G import Vid2VidModelG
    from vid2vid_amd.models.vid2vid_model_D import Vid2VidModelD
    G = Vid2VidModelG(); G.initialize(opt)
    D = Vid2VidModelD(); D.initialize(opt)
    return G, D


def test_models_pass_the_options_to_every_training_optimizer(dry_run, tmp_path):
    names = ["optimizer_D", "optimizer_D_T0", "optimizer_D_T1", "optimizer_G"]
    G, D = _models(_train_opt(tmp_path))
    for o in (G.optimizer_G, D.optimizer_D, D.optimizer_D_T0, D.optimizer_D_T1):
        assert not hasattr(o, "_guard") and not o.capturable and _recorded(o.step) == ["adam_step"]
    assert G.grad_guard_stats() == {} and D.grad_guard_stats() == {}

    for kw in (dict(max_grad_norm=4.0), dict(skip_nonfinite_grads=True), dict(max_grad_norm=4.0, skip_nonfinite_grads=True, ema_decay=0.9)):
        G, D = _models(_train_opt(tmp_path, **kw))
        stats = dict(G.grad_guard_stats(), **D.grad_guard_stats())
        assert sorted(stats) == names
        for name in names:
            o = getattr(G if name == "optimizer_G" else D, name)
            assert o.guarded and o.capturable
            assert o.max_grad_norm == kw.get("max_grad_norm", 0.0) and o.skip_nonfinite == kw.get("skip_nonfinite_grads", False)
            last = "adam_step_dev_guard_ema" if (name == "optimizer_G" and "ema_decay" in kw) else "adam_step_dev_guard"
            assert _recorded(o.step) == ["grad_sumsq", "guard_finalize", last], name
            assert stats[name] == {"grad_norm": 0.0, "clip_coef": 1.0, "skipped": 0, "applied": 0, "nonfinite": 0}

    # the face discriminator's parameters live in optimizer_D's flat buffer: the same guard covers them
    G, D = _models(_train_opt(tmp_path, skip_nonfinite_grads=True, niter_fix_global=1, fix_update_fixed_params=True))
    live, numel = G.optimizer_G, G.optimizer_G.flat.numel
    G.update_fixed_params()                                # FusedAdam.rebuild over all scales: the settings stay
    assert G.optimizer_G is live and live.flat.numel > numel and live.guarded and live.skip_nonfinite
    assert _recorded(live.step) == ["grad_sumsq", "guard_finalize", "adam_step_dev_guard"]
    # the reference-compatible update_fixed_params leaves a stand-in in optimizer_G: the stats follow the stepping optimizer
    G, D = _models(_train_opt(tmp_path, max_grad_norm=1.0, niter_fix_global=1))
    G.update_fixed_params()
    assert list(G.grad_guard_stats()) == ["optimizer_G"]
