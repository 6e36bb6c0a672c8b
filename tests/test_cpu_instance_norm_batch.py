"""CPU-side checks of InstanceNorm2d at batch > 1 (csrc/instance_norm.hip): C ABI surface, argument validation / dry run,
plan recording, and the engine lowering in record-only mode (no launch)."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT

NEW = ("v2v_in_stats", "v2v_in_apply", "v2v_in_backward")
EINVAL = -1
F32, BF16 = 0, 1


def _header_args(header, name):
    m = re.search(r"\bint(?:64_t)?\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
    assert m, "%s is not declared in include/v2v_hip.h" % name
    return [a for a in m.group(1).split(",") if a.strip()]


def test_library_exports_and_header_declares_the_entry_points():
    from vid2vid_amd import lib
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    for name in NEW + ("v2v_in_groups", "v2v_in_workspace_bytes", "v2v_in_ticket_words"):
        assert hasattr(lib.lib, name), "libv2v_hip.so does not export %s" % name
        assert name in lib.exported_symbols()
        assert len(_header_args(header, name)) == len(lib.PROTOTYPES[name][1]), name
    # the block cites what it stands for in the reference
    block = header[header.index("InstanceNorm2d at any batch size"):header.index("int v2v_in_backward")]
    assert "get_norm_layer" in block and "models/networks.py:23-30" in block and "nn.InstanceNorm2d" in block
    assert "training" in block


def test_new_source_is_in_the_makefile_and_never_imports_the_oracle():
    mk = open(os.path.join(ROOT, "vid2vid_amd", "csrc", "Makefile")).read()
    assert "instance_norm.hip" in mk
    src = open(os.path.join(ROOT, "vid2vid_amd", "csrc", "instance_norm.hip")).read()
    assert "oracle" not in src and "atomicAdd" not in src          # no floating-point atomics: fixed-order reductions


@pytest.fixture
def dry_run():
    from vid2vid_amd.lib import lib
    prev = lib.v2v_set_dry_run(1)
    yield lib
    lib.v2v_set_dry_run(prev)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_workspace_helpers():
    from vid2vid_amd.lib import lib
    assert lib.v2v_in_groups(0, 8, 1) == 0 and lib.v2v_in_groups(64, 0, 1) == 0 and lib.v2v_in_groups(64, 8, 0) == 0
    for HW, Cc, N in ((1, 3, 1), (252, 16, 2), (320, 1027, 5), (2048, 512, 4), (1 << 19, 64, 2)):
        g = lib.v2v_in_groups(HW, Cc, N)
        assert 1 <= g <= 256 and g <= -(-HW // 64)
        assert lib.v2v_in_workspace_bytes(HW, Cc, N) == N * g * Cc * 16 + N * Cc * 16 + N * Cc * 8
        assert lib.v2v_in_ticket_words(Cc, N) == N * -(-Cc // 64)
    assert lib.v2v_in_workspace_bytes(0, 8, 1) == 0 and lib.v2v_in_ticket_words(8, 0) == 0


def test_in_stats_validates_geometry(dry_run):
    lib = dry_run
    p = _ptr(torch.zeros(1 << 16))
    good = dict(raw=p, dt=F32, cs=16, ss=p, ws=p, tk=p, N=2, HW=252, C=16)

    def call(**kw):
        a = dict(good); a.update(kw)
        return lib.v2v_in_stats(a["raw"], a["dt"], a["cs"], None, None, 1e-5, a["ss"], a["ws"], a["tk"], a["N"], a["HW"], a["C"], None)
    assert call() == 0, lib.v2v_last_error()
    assert call(C=13) == 0 and call(dt=BF16) == 0 and call(N=1) == 0
    for bad in (dict(N=0), dict(N=-2), dict(C=0), dict(C=-1), dict(HW=0), dict(ss=None), dict(raw=None), dict(ws=None), dict(tk=None),
                dict(cs=12), dict(cs=18), dict(dt=BF16, cs=20), dict(dt=7), dict(N=70000)):
        assert call(**bad) == EINVAL, bad
    assert b"in_stats" in lib.v2v_last_error()


def test_in_apply_validates_geometry(dry_run):
    lib = dry_run
    p = _ptr(torch.zeros(1 << 16))
    good = dict(raw=p, rdt=F32, cs_raw=16, ss=p, a0=None, a1=None, y=p, x3=None, N=2, HW=252, C=16, cs=16, act=1, dt=F32)

    def call(**kw):
        a = dict(good); a.update(kw)
        return lib.v2v_in_apply(a["raw"], a["rdt"], a["cs_raw"], a["ss"], a["a0"], a["a1"], a["y"], a["x3"], a["N"], a["HW"], a["C"],
                                a["cs"], a["act"], 0.2, a["dt"], None)
    assert call() == 0, lib.v2v_last_error()
    assert call(a0=p, a1=p, x3=p) == 0 and call(dt=BF16, rdt=BF16) == 0 and call(C=13) == 0
    for act in range(5):
        assert call(act=act) == 0
    for bad in (dict(N=0), dict(C=0), dict(HW=-1), dict(ss=None), dict(raw=None), dict(y=None), dict(cs_raw=12), dict(cs=12),
                dict(dt=BF16, cs=20), dict(act=5), dict(act=-1), dict(x3=p, dt=BF16), dict(x3=p, C=12, cs=16), dict(x3=p, C=14, cs=14)):
        assert call(**bad) == EINVAL, bad
    assert b"in_apply" in lib.v2v_last_error()


def test_in_backward_validates_geometry(dry_run):
    lib = dry_run
    p = _ptr(torch.zeros(1 << 16))
    good = dict(dy=p, raw=p, cs_raw=16, st=p, dr=p, cs_out=16, dg=None, db=None, ws=p, tk=p, N=3, HW=320, C=16, cs=16, act=2, dt=F32)

    def call(**kw):
        a = dict(good); a.update(kw)
        return lib.v2v_in_backward(a["dy"], a["raw"], a["cs_raw"], a["st"], a["dr"], a["cs_out"], a["dg"], a["db"], 1, a["ws"], a["tk"],
                                   a["N"], a["HW"], a["C"], a["cs"], a["act"], 0.2, a["dt"], None)
    assert call() == 0, lib.v2v_last_error()
    assert call(dg=p, db=p) == 0 and call(dt=BF16) == 0 and call(C=13) == 0       # affine=True is handled, not refused
    for bad in (dict(N=0), dict(C=0), dict(HW=0), dict(st=None), dict(dy=None), dict(raw=None), dict(dr=None), dict(ws=None),
                dict(tk=None), dict(cs_raw=12), dict(cs=12), dict(cs_out=12), dict(cs_out=18), dict(act=3), dict(act=4), dict(dt=3)):
        assert call(**bad) == EINVAL, bad
    assert b"in_backward" in lib.v2v_last_error()


def test_dry_run_touches_no_memory(dry_run):
    """Dry run returns 0 for valid arguments without dereferencing any of them: the pointers here are not mapped."""
    lib = dry_run
    bogus = C.c_void_p(0x10000)
    assert lib.v2v_in_stats(bogus, F32, 16, None, None, 1e-5, bogus, bogus, bogus, 2, 252, 16, None) == 0
    assert lib.v2v_in_apply(bogus, F32, 16, bogus, None, None, bogus, None, 2, 252, 16, 16, 1, 0.0, F32, None) == 0
    assert lib.v2v_in_backward(bogus, bogus, 16, bogus, bogus, 16, None, None, 1, bogus, bogus, 2, 252, 16, 16, 1, 0.0, F32, None) == 0


def test_entry_points_record_into_a_plan(dry_run):
    lib = dry_run
    p = _ptr(torch.zeros(1 << 16))
    plan = lib.v2v_plan_create()
    try:
        assert lib.v2v_plan_begin_record(plan) == 0
        assert lib.v2v_in_stats(p, F32, 16, None, None, 1e-5, p, p, p, 2, 252, 16, None) == 0
        assert lib.v2v_in_apply(p, F32, 16, p, None, None, p, None, 2, 252, 16, 16, 1, 0.0, F32, None) == 0
        assert lib.v2v_in_backward(p, p, 16, p, p, 16, None, None, 1, p, p, 2, 252, 16, 16, 1, 0.0, F32, None) == 0
        assert lib.v2v_plan_end_record(plan) == 0
        names = [lib.v2v_plan_op_name(plan, i).decode() for i in range(lib.v2v_plan_num_ops(plan))]
        assert names == ["in_stats", "in_apply", "in_backward"]
    finally:
        lib.v2v_plan_destroy(plan)


def test_engine_lowers_a_batched_instance_norm_group_in_record_only_mode():
    """Engine._norm_params(InstanceNorm2d, N=2) no longer raises, and a batch-2 group records conv -> in_stats -> in_apply
    (no statistics finalize over the whole launch); batch 1 keeps the BatchNorm machinery."""
    from vid2vid_amd import lib as L
    from vid2vid_amd.engine import Engine, Act, Plan
    prev = L.lib.v2v_get_dry_run()
    try:
        eng = Engine("cpu", L.F32, record_only=True)
        norm = nn.InstanceNorm2d(16)
        gamma, beta, eps, _, rm, rv = eng._norm_params(norm, 2)
        assert gamma is None and beta is None and rm is None and rv is None and eps == norm.eps
        assert eng.inst_batched(norm, 2) and not eng.inst_batched(norm, 1) and not eng.inst_batched(nn.BatchNorm2d(16), 2)
        with pytest.raises(RuntimeError, match="batch-wide"):
            eng._batchwide_params(norm, 2)
        conv = nn.Conv2d(16, 16, 3)
        for N, want in ((2, ["in_stats", "in_apply"]), (1, ["bn_apply"])):
            x = Act(torch.zeros(N, 14, 18, 16), 16)
            plan = Plan()
            with torch.no_grad():
                eng.plan = plan
                with plan:
                    y = eng.conv_group(x, conv, L.PAD_REFLECT, 1, norm, L.ACT_RELU, 0.0, add0=x, label="g")
                eng.plan = None
            names = [L.lib.v2v_plan_op_name(plan.h, i).decode() for i in range(plan.num_ops)]
            assert tuple(y.t.shape) == (N, 14, 18, 16)
            assert any(n.startswith("conv") for n in names) and names[-len(want):] == want, names
            assert ("in_stats" in names) == (N > 1)
    finally:
        L.lib.v2v_set_dry_run(prev)
