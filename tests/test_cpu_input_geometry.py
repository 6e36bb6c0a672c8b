"""uint8 inputs at source size (opt.input_geometry): what can be checked without a GPU -- the restatement of the index
map against Pillow itself, the option's refusals on the dry-run backend, the ABI and its argument checks, the defaults and the
entry table the host builds for a call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from input_geometry_common import box, gather, index_maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source, destination) extents along one axis
PAIRS = [(1920, 1024), (1080, 512), (1280, 512), (720, 256), (2048, 1024), (1000, 333), (455, 256), (97, 64), (50, 128),
         (1914, 1024), (101, 96), (33, 64)]


# ------------------------------------------------------------------ 1. the restatement against Pillow
def _pil_pipeline(img, geom):
    """The reference's transform of an input map (data/base_dataset.py:160-175 with method=Image.NEAREST), on a PIL image."""
    from PIL import Image
    img = img.resize(tuple(geom["new_size"]), Image.NEAREST)
    tw, th = geom.get("crop_size", (0, 0))
    if (tw, th) != (0, 0):
        ow, oh = img.size
        x1, y1 = geom["crop_pos"]
        if ow > tw or oh > th:
            img = img.crop((x1, y1, min(ow, x1 + tw), min(oh, y1 + th)))
    if geom.get("flip", False):
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return img


def _pil_frames(src, geom):
    """src (Hs, Ws, C) uint8, C in {1, 3, 6}: mode L, RGB, or two RGB images side by side in the channel dimension."""
    from PIL import Image
    Cc = src.shape[-1]
    if Cc == 1:
        return np.asarray(_pil_pipeline(Image.fromarray(src[..., 0], "L"), geom))[..., None]
    parts = [np.asarray(_pil_pipeline(Image.fromarray(np.ascontiguousarray(src[..., c:c + 3]), "RGB"), geom)) for c in range(0, Cc, 3)]
    return np.concatenate(parts, axis=-1)


def _check_against_pil(Hs, Ws, Cc, geom, seed):
    from vid2vid_amd import visual
    src = np.random.default_rng(seed).integers(0, 256, (Hs, Ws, Cc), dtype=np.uint8)
    want = _pil_frames(src, geom)
    got = gather(src, geom)
    assert got.shape == want.shape, (got.shape, want.shape, geom)
    assert np.array_equal(got, want), geom
    # the product's host side: the size it announces and the words it hands the launch
    x1, y1, W, H = box(geom)
    assert tuple(visual.geometry_size(geom)) == (H, W) == want.shape[:2]
    assert tuple(visual.geometry_words(geom)) == (geom["new_size"][0], geom["new_size"][1], x1, y1, int(geom.get("flip", False)), H, W)
    return got


@pytest.mark.parametrize("pair", PAIRS)
def test_restatement_equals_pillow_resize_on_every_pair(pair):
    pytest.importorskip("PIL")
    s, d = pair
    for Cc in (1, 3, 6):
        # the pair along the width, then along the height; the other axis 7 -> 5 (a downscale) or 5 -> 7
        _check_against_pil(7, s, Cc, dict(new_size=(d, 5)), seed=s + Cc)
        _check_against_pil(s, 5, Cc, dict(new_size=(7, d), flip=True), seed=s + d + Cc)
    # every index of the pair, not only the bytes that happen to differ: a ramp whose value is the source index
    sy, sx = index_maps(1, s, dict(new_size=(d, 1)))
    from PIL import Image
    lo = np.asarray(Image.fromarray((np.arange(s) % 256).astype(np.uint8)[None, :], "L").resize((d, 1), Image.NEAREST))[0]
    hi = np.asarray(Image.fromarray((np.arange(s) // 256).astype(np.uint8)[None, :], "L").resize((d, 1), Image.NEAREST))[0]
    assert np.array_equal(lo.astype(np.int64) + 256 * hi.astype(np.int64), sx) and sy.tolist() == [0]


@pytest.mark.parametrize("flip", [False, True])
def test_restatement_equals_pillow_with_crops_and_flip(flip):
    pytest.importorskip("PIL")
    geoms = [
        dict(new_size=(72, 40), crop_size=(64, 32), crop_pos=(5, 3)),          # the box inside the frame
        dict(new_size=(72, 40), crop_size=(64, 32), crop_pos=(20, 12)),        # x1 + tw > ow and y1 + th > oh: clipped
        dict(new_size=(72, 40), crop_size=(64, 64), crop_pos=(20, 0)),         # oh <= th but ow > tw: still cropped, height clipped
        dict(new_size=(64, 32), crop_size=(64, 32), crop_pos=(0, 0)),          # ow <= tw and oh <= th: no crop
        dict(new_size=(64, 32), crop_size=(96, 64), crop_pos=(0, 0)),          # the same with a larger box
        dict(new_size=(64, 32), crop_size=(0, 0), crop_pos=(0, 0)),            # get_img_params without a crop stage
        dict(new_size=(64, 32)),                                               # the keys missing
    ]
    for i, geom in enumerate(geoms):
        geom = dict(geom, flip=flip)
        for Cc in (1, 3, 6):
            got = _check_against_pil(45, 100, Cc, geom, seed=17 * i + Cc)
            assert got.shape[:2] == [(32, 64), (28, 52), (40, 52), (32, 64), (32, 64), (32, 64), (32, 64)][i]
    # crop_pos is not looked at without a crop stage
    from vid2vid_amd import visual
    assert visual.geometry_words(dict(new_size=(64, 32), crop_size=(0, 0), crop_pos=(-7, 900), flip=flip))[2:4] == (0, 0)
    assert visual.geometry_words(dict(new_size=(64, 32), crop_pos=(-7, 900), flip=flip))[2:4] == (0, 0)


def test_a_drop_in_caller_passes_get_img_params_through():
    """numpy integers (crop_x comes out of np.maximum) and lists are taken as they are."""
    from vid2vid_amd import visual
    geom = {"new_size": (np.int64(72), 40), "crop_size": [64, 32], "crop_pos": (np.int64(5), np.int32(3)), "flip": np.bool_(True)}
    assert visual.geometry_words(geom) == (72, 40, 5, 3, 1, 32, 64)
    assert visual.geometry_size(geom) == (32, 64)


# ------------------------------------------------------------------ 2. every refusal, on the dry-run backend
@pytest.fixture
def record_only():
    from vid2vid_amd import networks as N
    if torch.cuda.is_available():
        pytest.skip("dry-run check on a CPU host")
    N.set_record_only(True)
    yield
    N.set_record_only(False)
    N._ENGINES.clear()


def _model(**kw):
    from vid2vid_amd.options import make_opt
    from vid2vid_amd.models import create_model
    d = dict(label_nc=0, input_nc=6, use_instance=False, fg=False, use_real_img=True, random_init_ok=True, precision="bf16",
             gpu_ids=[], ngf=8, n_blocks=2, n_downsample_G=2, inputs_u8=True, inputs_u8_slots=True)
    d.update(kw)
    return create_model(make_opt(**d))


H, W, HS, WS = 16, 32, 23, 50
GEOM = dict(new_size=(36, 20), crop_size=(32, 16), crop_pos=(2, 3), flip=False)
BAD_GEOMETRIES = [
    dict(GEOM, new_size=(0, 20)), dict(GEOM, new_size=(36, -4)), dict(GEOM, new_size=(16385, 20)), dict(GEOM, new_size=(36, 16385)),
    dict(GEOM, crop_pos=(-1, 3)), dict(GEOM, crop_pos=(2, -1)), dict(GEOM, crop_pos=(36, 3)), dict(GEOM, crop_pos=(2, 20)),
    dict(GEOM, flip=1), dict(GEOM, flip=None), dict(GEOM, flip="no"),
]


def _src(B, t=3, hs=HS, ws=WS, seed=0):
    return torch.randint(0, 256, (B, t, hs, ws, 6), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _first(B):
    return torch.zeros(B, 2, 3, H, W)


def test_refusals_before_a_sequence_starts(record_only):
    from vid2vid_amd import visual
    assert visual.geometry_size(GEOM) == (H, W)
    m = _model(input_geometry=GEOM)

    def refused(A, **kw):
        with pytest.raises(ValueError):
            m.inference(A, _first(A.shape[0]), None, **kw)
        assert getattr(m, "fake_B_prev", None) is None and m._active_plan is None and not m._plans

    for bad in BAD_GEOMETRIES:
        m.opt.input_geometry = bad
        refused(_src(1))
        with pytest.raises(ValueError):
            visual.geometry_words(bad)
    m.opt.input_geometry = GEOM
    refused(_src(1).float())                                                   # not uint8
    refused(_src(1)[0])                                                        # not 5-D
    refused(_src(1, hs=16385, ws=1))                                           # Hs above 16384
    refused(_src(1, hs=1, ws=16385))                                           # Ws above 16384
    m.opt.input_geometry = [GEOM]
    refused(_src(2))                                                           # a list of another length
    m.opt.input_geometry = [GEOM, GEOM, GEOM]
    refused(_src(2))
    m.opt.input_geometry = [GEOM, dict(new_size=(36, 20))]                     # stream 1 at 20x36, stream 0 at 16x32
    refused(_src(2))
    # slot and pool calls without opt.inputs_u8_slots
    m.opt.input_geometry = GEOM
    m.opt.inputs_u8_slots = False
    refused(_src(2), active=[0])
    refused(_src(2), restart=[1])
    m.opt.compact_streams = True
    refused(_src(2))
    m.opt.compact_streams = False
    m.opt.inputs_u8_slots = True
    # the option without opt.inputs_u8
    m.opt.inputs_u8 = False
    refused(_src(1))
    with pytest.raises(ValueError, match="input_geometry"):
        m.inference(torch.rand(1, 3, 6, H, W), _first(1), None)
    m.opt.inputs_u8 = True
    # and then it runs
    fake, last = m.inference(_src(1), _first(1), None)
    assert tuple(fake.shape) == (1, 3, H, W) and tuple(last.shape) == (6, H, W)
    assert tuple(m._active_plan.win_u8.shape) == (1, 3, H, W, 6) and (m._active_plan.H, m._active_plan.W) == (H, W)


def test_a_label_model_refuses_the_option(record_only):
    m = _model(label_nc=35, input_nc=3, inputs_u8=False, inputs_u8_slots=False, input_geometry=GEOM)
    for u8 in (False, True):
        m.opt.inputs_u8 = u8
        with pytest.raises(ValueError):
            m.inference(torch.zeros(1, 3, HS, WS, 1, dtype=torch.uint8), torch.zeros(1, 2, 3, H, W), None)
        assert getattr(m, "fake_B_prev", None) is None and m._active_plan is None and not m._plans


def test_refusals_leave_a_running_sequence_and_its_window_untouched(record_only):
    """B = 2 in a slot plan.  Nothing executes on this backend, so the window holds the sentinel written here: a refused call must
    neither stage into it (copy_, zero_) nor rewrite the launch's tables."""
    m = _model(input_geometry=[GEOM, dict(new_size=(32, 16), flip=True)])
    m.inference(_src(2), _first(2), None, active=[0, 1])
    fp = m._active_plan
    assert fp.slots and tuple(fp.win_u8.shape) == (2, 3, H, W, 6)
    fp.win_u8.fill_(0x5A)
    tables = fp._gather[0].clone()
    prev = [p.clone() for p in m.fake_B_prev]

    def refused(A, first=None, **kw):
        kw.setdefault("active", [0, 1])
        with pytest.raises(ValueError):
            m.inference(A, first, None, **kw)
        assert m._active_plan is fp and bool((fp.win_u8 == 0x5A).all()) and torch.equal(fp._gather[0], tables)
        assert all(torch.equal(a, b) for a, b in zip(m.fake_B_prev, prev))

    good = m.opt.input_geometry
    for bad in BAD_GEOMETRIES:
        m.opt.input_geometry = [good[0], bad]
        refused(_src(2, t=1))
        m.opt.input_geometry = bad
        refused(_src(2, t=1))
    m.opt.input_geometry = dict(new_size=(64, 32))                             # another size than the running plan's
    refused(_src(2, t=1))
    m.opt.input_geometry = [good[0], dict(new_size=(64, 32))]                  # ... for one stream
    refused(_src(2, t=1))
    m.opt.input_geometry = [good[0]]
    refused(_src(2, t=1))
    m.opt.input_geometry = good
    refused(_src(2, t=1).float())
    refused(_src(2, t=1)[:, 0])
    refused(_src(2, t=1, hs=16385, ws=1))
    refused(_src(2, t=2))                                                      # the rules for t stay
    refused(_src(2, t=1), restart=[1])                                         # a restarted stream brings its whole window
    refused(_src(2, t=3), _first(2), restart=[1], active=[0])                  # restarted and idle
    m.opt.inputs_u8_slots = False
    refused(_src(2, t=1))
    m.opt.inputs_u8_slots = True
    m.opt.inputs_u8 = False
    refused(_src(2, t=1))
    m.opt.inputs_u8 = True
    m.inference(_src(2, t=1), None, None, active=[0, 1])                       # the sequence goes on
    assert m._active_plan is fp and not torch.equal(fp._gather[0], tables)


# ------------------------------------------------------------------ 3. the ABI
_CTYPE = {"const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "const int32_t*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32}


def test_entry_point_signature_header_and_export_agree():
    from vid2vid_amd import lib as L
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    args = [a.strip() for a in re.search(r"\bint\s+v2v_gather_frames_u8\s*\(([^)]*)\)", header).group(1).split(",")]
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["src", "F", "Hs", "Ws", "dst", "D", "H", "W", "C", "entries", "E", "geoms", "G", "stream"]
    types = [_CTYPE[a[:a.rindex(n)].replace(" *", "*").strip()] for a, n in zip(args, names)]
    res, argtypes = L.PROTOTYPES["v2v_gather_frames_u8"]
    assert res is C.c_int and list(argtypes) == types
    assert "v2v_gather_frames_u8" in L.exported_symbols() and list(L.lib.v2v_gather_frames_u8.argtypes) == types


def test_entry_point_argument_checks_answer_on_the_host():
    """Host buffers stand in for device pointers; dry-run mode validates and returns, so nothing is ever dereferenced."""
    from vid2vid_amd import lib as L
    F, Hs, Ws, D, H_, W_, Cc, E, G = 3, 9, 11, 4, 6, 8, 6, 5, 2
    al = lambda buf, off=0: C.c_void_p(((C.addressof(buf) + 15) & ~15) + off)
    src = (C.c_uint8 * (F * Hs * Ws * 32 + 16))()                               # room for the widest C tried below
    dst = (C.c_uint8 * (D * H_ * W_ * 32 + 16))()
    ent = (C.c_int32 * (4 * E + 4))()
    geo = (C.c_int32 * (8 * G + 4))()
    base = dict(src=al(src), F=F, Hs=Hs, Ws=Ws, dst=al(dst), D=D, H=H_, W=W_, C=Cc, entries=al(ent), E=E, geoms=al(geo), G=G)

    def call(**kw):
        a = dict(base, **kw)
        return L.lib.v2v_gather_frames_u8(a["src"], a["F"], a["Hs"], a["Ws"], a["dst"], a["D"], a["H"], a["W"], a["C"], a["entries"],
                                          a["E"], a["geoms"], a["G"], None)
    prev = L.lib.v2v_set_dry_run(1)
    try:
        assert call() == 0 and call(E=0) == 0 and call(C=1) == 0 and call(C=32) == 0
        assert call(src=al(src, 1), dst=al(dst, 3)) == 0                        # no alignment is asked of the frames
        bad = [dict(src=None), dict(dst=None), dict(entries=None), dict(geoms=None), dict(C=0), dict(C=33), dict(C=-1), dict(E=-1)]
        bad += [{k: v} for k in ("Hs", "Ws", "H", "W") for v in (0, -1, 16385)]
        bad += [dict(F=0), dict(D=0), dict(G=0)]
        bad += [dict(dst=al(src)), dict(dst=al(src, F * Hs * Ws * Cc - 1)), dict(src=al(dst, D * H_ * W_ * Cc - 1))]      # overlaps
        bad += [dict(entries=al(ent, 4)), dict(geoms=al(geo, 8))]               # tables off their 16-byte alignment
        for kw in bad:
            assert call(**kw) == -1, kw
            assert b"gather_frames_u8" in L.lib.v2v_last_error(), kw
        # source and destination side by side do not overlap
        assert call(F=1, src=al(dst, D * H_ * W_ * Cc), Hs=1, Ws=1) == 0
    finally:
        L.lib.v2v_set_dry_run(prev)


# ------------------------------------------------------------------ 4. defaults and the entry table
def test_option_default():
    from vid2vid_amd.options import make_opt
    assert make_opt().input_geometry is None
    assert make_opt(input_geometry=GEOM).input_geometry is GEOM


def test_entry_table_function():
    from vid2vid_amd.visual import gather_entries
    # streams 0 (restarted), 1 (steady), 2 (idle) of B = 3, tG = 3, the call brings t = 3 frames per stream
    assert gather_entries(3, 3, [0, 1], [0], True) == [[0, 0, 0, 0], [1, 1, 0, 0], [2, 2, 0, 0], [5, 5, 1, 0]]
    assert gather_entries(3, 3, [0, 1], [0], False) == [[0, 0, 0, 0], [1, 1, 0, 0], [2, 2, 0, 0], [5, 5, 0, 0]]
    # t = 1: frame b of the call into slot tG - 1 of window b
    assert gather_entries(1, 3, [0, 2], [], True) == [[0, 2, 0, 0], [2, 8, 2, 0]]
    assert gather_entries(1, 3, [], [], True) == []
    with pytest.raises(ValueError):
        gather_entries(1, 3, [0], [0], True)


@pytest.mark.parametrize("pool", [False, True])
def test_host_builds_the_entry_table_of_a_call(record_only, pool):
    """One restarted, one steady and one idle stream: tG + 1 entries and none for the idle stream; the geometry table has a row per
    stream.  Slot plan and pool plan (where window b is the pool's slot b whatever the plan's row count)."""
    tG = 3
    geoms = [GEOM, dict(new_size=(32, 16), flip=True), dict(new_size=(64, 20), crop_size=(32, 16), crop_pos=(32, 4), flip=False)]
    m = _model(input_geometry=geoms, compact_streams=pool)
    m.inference(_src(3), _first(3), None)                                      # every stream starts: 3 tG entries
    ent, geo = m._active_plan.gather_last
    assert ent.dtype == geo.dtype == torch.int32 and tuple(ent.shape) == (3 * tG, 4) and tuple(geo.shape) == (3, 8)
    assert ent.tolist() == [[f, f, f // tG, 0] for f in range(3 * tG)]
    assert geo.tolist() == [[36, 20, 2, 3, 0, 0, 0, 0], [32, 16, 0, 0, 1, 0, 0, 0], [64, 20, 32, 4, 0, 0, 0, 0]]
    assert ent.data_ptr() % 16 == 0 and geo.data_ptr() % 16 == 0
    m.inference(_src(3), _first(3), None, restart=[1], active=[0, 1])          # 0 steady, 1 restarted, 2 idle
    fp = m._active_plan
    ent, geo = fp.gather_last
    assert (fp.pool is not None) == pool and fp.B == (2 if pool else 3)
    assert ent.tolist() == [[2, 2, 0, 0], [3, 3, 1, 0], [4, 4, 1, 0], [5, 5, 1, 0]] and len(ent) == tG + 1
    assert not any(6 <= e[0] or 6 <= e[1] or e[2] == 2 for e in ent.tolist())
    assert tuple(geo.shape) == (3, 8)
    m.inference(_src(3, t=1), None, None, active=[1, 2])                       # t = 1, stream 0 idle
    ent, _ = m._active_plan.gather_last
    assert ent.tolist() == [[1, 5, 1, 0], [2, 8, 2, 0]]
    # one dict for every stream: one row
    m.opt.input_geometry = GEOM
    m.inference(_src(3, t=1), None, None, active=[0])
    ent, geo = m._active_plan.gather_last
    assert ent.tolist() == [[0, 2, 0, 0]] and geo.tolist() == [[36, 20, 2, 3, 0, 0, 0, 0]]
    # an empty call stages nothing
    keep = m._active_plan.gather_last
    m.inference(_src(3, t=1), None, None, active=[])
    assert m._active_plan.gather_last is keep


def test_resample_u8_argument_rules():
    from vid2vid_amd import visual
    from vid2vid_amd import lib as L
    src = torch.zeros(2, HS, WS, 3, dtype=torch.uint8)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="device memory"):                 # host frames outside the dry-run backend
            visual.resample_u8(src, GEOM)
    prev = L.lib.v2v_set_dry_run(1)
    try:
        out = visual.resample_u8(src, GEOM)
        assert tuple(out.shape) == (2, H, W, 3) and out.dtype == torch.uint8
        assert visual.resample_u8(src, GEOM, out=out) is out
        for bad in (src.float(), src[0], torch.zeros(2, HS, WS, 33, dtype=torch.uint8)):
            with pytest.raises(ValueError):
                visual.resample_u8(bad, GEOM)
        with pytest.raises(ValueError):
            visual.resample_u8(src, GEOM, out=torch.zeros(2, H, W + 1, 3, dtype=torch.uint8))
        with pytest.raises(ValueError):
            visual.resample_u8(src, dict(GEOM, flip=1))
    finally:
        L.lib.v2v_set_dry_run(prev)
