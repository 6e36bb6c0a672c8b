"""--add_face_disc (the pose2body recipes) on a GPU-less host: the face window arithmetic against the reference's
get_face_region, netD_f's checkpoint keys and seeded initialisation against the reference's, and -- with the backend in
dry-run mode (every launch argument-checked, nothing executed) -- loss names, optimizer order, checkpoints and the role
split (netD_f on D-rank 0: broadcast at start-up, saved once)."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, GOLDEN
from face_disc_common import CASES, FINE, H, W, ORDER, face_region_torch, make_inputs, window_from_box

REF = os.environ.get("V2V_REFERENCE", "/root/reference")
HAVE_REF = os.path.isfile(os.path.join(REF, "models", "vid2vid_model_D.py"))
FACE_LOSSES = ["G_f_GAN", "G_f_GAN_Feat", "D_f_real", "D_f_fake"]
LOSS_NAMES = ["G_VGG", "G_GAN", "G_GAN_Feat", "D_real", "D_fake", "G_Warp", "F_Flow", "F_Warp", "W"] + FACE_LOSSES


def _pose_opt(ckpt, **kw):
    from vid2vid_amd.options import make_opt
    d = dict(isTrain=True, label_nc=0, input_nc=6, add_face_disc=True, num_D=3, ndf=8, no_vgg=True, loadSize=FINE,
             fineSize=FINE, n_scales_temporal=1, precision="fp32", random_init_ok=True, checkpoints_dir=ckpt, name="pose")
    d.update(kw)
    return make_opt(**d)


@pytest.fixture
def dry():
    from vid2vid_amd import networks as N
    N.set_record_only(True)
    yield
    N.set_record_only(False)


def _model_D(opt):
    from vid2vid_amd.models.vid2vid_model_D import Vid2VidModelD
    D = Vid2VidModelD()
    D.initialize(opt)
    return D


# ---------------------------------------------------------------------------------------------- window arithmetic
def test_window_restatement_matches_the_golden_regions():
    g = np.load(os.path.join(GOLDEN, "face_disc_pose_64x128.npz"))
    for case in CASES:
        t = make_inputs(case)
        got = face_region_torch(t["real_A"], FINE, openpose=case == "openpose")
        want = tuple(int(v) for v in g["%s.region" % case])
        assert tuple(-1 if v is None else v for v in got) == want, case


def _reference_D(openpose=False, fine=FINE, seed=80):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden import install_shims
    install_shims()
    # the reference's `util` package (options/base_options.py: `from util import util`) shares its name with tests/util.py
    ours = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "util" or k.startswith("util.")}
    try:
        from options.train_options import TrainOptions
        from models.vid2vid_model_D import Vid2VidModelD
    finally:
        for k in [k for k in sys.modules if k == "util" or k.startswith("util.")]:
            del sys.modules[k]
        sys.modules.update(ours)
    argv = sys.argv
    sys.argv = ["train.py", "--name", "pose", "--dataset_mode", "pose", "--label_nc", "0", "--input_nc", "6", "--add_face_disc",
                "--num_D", "3", "--ndf", "8", "--no_vgg", "--gpu_ids", "-1", "--checkpoints_dir", tempfile.mkdtemp(),
                "--loadSize", str(fine), "--fineSize", str(fine), "--n_scales_temporal", "1"] + (["--openpose_only"] if openpose else [])
    try:
        opt = TrainOptions().parse(save=False)
    finally:
        sys.argv = argv
    opt.gpu_ids = [-1]
    opt.n_gpus_gen = 1
    torch.manual_seed(seed)
    D = Vid2VidModelD()
    D.initialize(opt)
    return D


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference tree (build container)")
@pytest.mark.parametrize("openpose", [False, True])
def test_window_arithmetic_equals_reference_get_face_region(openpose):
    """The box -> window arithmetic (what v2v_face_window's finalize step computes, restated) against the reference's own
    get_face_region on seeded random masks and edge cases, for several frame / crop sizes."""
    for fine, h, w in ((128, 64, 128), (512, 512, 256), (256, 64, 64)):
        D = _reference_D(openpose, fine)
        gen = torch.Generator().manual_seed(5 + fine + openpose)
        maps = []
        for k in range(12):
            a = torch.rand(2, 3, h, w, generator=gen) * 0.8
            m = torch.rand(2, h, w, generator=gen) < (0.0005 if k < 8 else 0.0)
            if k == 8:
                m[0, 0, 0] = True                                   # corner
            elif k == 9:
                m[1, h - 1, w - 1] = True                           # opposite corner
            elif k == 10:
                m[:] = True                                         # full mask
            elif k == 11:
                m[0, h // 2, 0] = True; m[1, 0, w // 2] = True      # union across frames
            if openpose:
                a[:, 0][m], a[:, 1][m], a[:, 2][m] = 0.2, -1.0, -0.6
            else:
                a[:, 2][m] = 0.95
            maps.append(a)
        maps.append(torch.rand(2, 3, h, w, generator=gen) * 0.8)   # empty mask
        for a in maps:
            want = D.get_face_region(a)
            assert face_region_torch(a, fine, openpose) == tuple(want)
            if want[0] is not None:
                mask = (a[:, 2] > 0.9) if not openpose else ((a[:, 0] > 0.19) & (a[:, 0] < 0.21) & (a[:, 1] < -0.99) &
                                                              (a[:, 2] > -0.61) & (a[:, 2] < -0.59))
                f = mask.nonzero()
                box = (int(f[:, 1].min()), int(f[:, 1].max()), int(f[:, 2].min()), int(f[:, 2].max()))
                assert window_from_box(*box, h, w, fine) == tuple(want)


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference tree (build container)")
def test_netD_f_keys_and_seeded_init_equal_the_reference(dry, tmp_path):
    ref = _reference_D(seed=80)
    torch.manual_seed(80)
    D = _model_D(_pose_opt(str(tmp_path)))
    mine, theirs = D.netD_f.state_dict(), ref.netD_f.state_dict()
    assert list(mine.keys()) == list(theirs.keys())
    for k in theirs:
        assert torch.equal(mine[k].cpu().contiguous(), theirs[k]), k
    assert D.netD_f.num_D == 1                                       # max(1, num_D - 2)


# ---------------------------------------------------------------------------------------------- dry-run model
def test_loss_names_optimizer_order_and_losses(dry, tmp_path):
    D = _model_D(_pose_opt(str(tmp_path)))
    assert D.loss_names == LOSS_NAMES
    want = [id(p) for p in list(D.netD.parameters()) + list(D.netD_f.parameters())]
    assert [id(p) for p in D.optimizer_D.flat.params] == want
    t = make_inputs("mid")
    t["fake_B"].requires_grad_(True)
    losses = D(0, [t[k] for k in ORDER])
    assert len(losses) == 13 and all(tuple(l.shape) == (1, 1) for l in losses)
    # get_losses adds the face terms exactly as the reference (:253-255)
    vals = {n: torch.full((1, 1), float(i + 1)) for i, n in enumerate(LOSS_NAMES)}
    loss_G, loss_D, loss_D_T, t_act = D.get_losses(vals, [], 0)
    assert float(loss_G) == 2 + 3 + 1 + 6 + 7 + 8 + 9 + 10 + 11
    assert float(loss_D) == (5 + 4) * 0.5 + (13 + 12) * 0.5
    assert loss_D_T == [] and t_act == 0


def test_crop_larger_than_the_frame_is_an_error(dry, tmp_path):
    D = _model_D(_pose_opt(str(tmp_path), fineSize=512, loadSize=512))
    with pytest.raises(ValueError):
        D.get_face_region(torch.zeros(1, 6, 64, 512))                # crop 128 > 64 rows


def test_face_window_arguments_are_checked():
    from vid2vid_amd import lib as L
    a = torch.zeros(2, 6, 64, 128)
    win = torch.zeros(8, dtype=torch.int32)
    p = lambda t: t.data_ptr()
    prev = L.lib.v2v_set_dry_run(1)
    try:
        assert L.lib.v2v_face_window(p(a), 2, 6, 64, 128, L.FACE_DENSEPOSE, 32, 32, p(win), None) == 0
        assert L.lib.v2v_face_window(p(a), 2, 6, 64, 128, 2, 32, 32, p(win), None) == -1         # unknown mode
        assert L.lib.v2v_face_window(p(a), 2, 2, 64, 128, 0, 32, 32, p(win), None) == -1         # fewer than 3 channels
        assert L.lib.v2v_face_window(p(a), 2, 6, 64, 128, 0, 128, 32, p(win), None) == -1        # crop taller than the frame
        assert L.lib.v2v_face_window(p(a), 2, 6, 64, 128, 0, 31, 32, p(win), None) == -1         # odd crop
        assert L.lib.v2v_face_window(p(a), 2, 6, 64, 128, 0, 32, 32, None, None) == -1
        y = torch.zeros(2, 32, 32, 12)
        assert L.lib.v2v_pack_concat_window_nhwc(p(a), 6, p(a), 3, 2, 64, 128, p(win), 32, 32, p(y), 12, L.F32, None) == 0
        assert L.lib.v2v_pack_concat_window_nhwc(p(a), 6, p(a), 3, 2, 64, 128, p(win), 32, 32, p(y), 10, L.F32, None) == -1
        assert L.lib.v2v_pack_concat_window_nhwc(p(a), 6, p(a), 3, 2, 64, 128, None, 32, 32, p(y), 12, L.F32, None) == -1
        assert L.lib.v2v_unpack_window_nchw(p(y), p(win), 2, 3, 64, 128, 32, 32, 12, 6, p(a), L.F32, None) == 0
        assert L.lib.v2v_unpack_window_nchw(p(y), p(win), 2, 3, 64, 128, 32, 32, 12, 10, p(a), L.F32, None) == -1
        assert L.lib.v2v_unpack_window_nchw(p(y), p(win), 2, 3, 64, 128, 32, 256, 12, 6, p(a), L.F32, None) == -1
    finally:
        L.lib.v2v_set_dry_run(prev)


def test_D_f_checkpoint_written_and_read_back(dry, tmp_path):
    torch.manual_seed(1)
    D = _model_D(_pose_opt(str(tmp_path)))
    with torch.no_grad():
        for p in D.netD_f.parameters():
            p.add_(0.5)
    D.save("latest")
    assert os.path.isfile(os.path.join(str(tmp_path), "pose", "latest_net_D_f.pth"))
    torch.manual_seed(2)
    D2 = _model_D(_pose_opt(str(tmp_path), continue_train=True))
    for k, v in D.netD_f.state_dict().items():
        assert torch.equal(D2.netD_f.state_dict()[k].cpu(), v.cpu()), k


def test_missing_D_f_checkpoint_is_tolerated(dry, tmp_path):
    """The 512p recipe loads the 256p checkpoint, which has no D_f (reference :56-57 through load_network)."""
    torch.manual_seed(1)
    D = _model_D(_pose_opt(str(tmp_path), add_face_disc=False))
    D.save("latest")
    _model_D(_pose_opt(str(tmp_path), continue_train=True))


# ---------------------------------------------------------------------------------------------- role split
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _role_worker(rank, world, port, ckpt, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from vid2vid_amd import networks as N, parallel
    N.set_record_only(True)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vid2vid_amd.models import create_model
        from vid2vid_amd.models.models import create_optimizer
        torch.manual_seed(300 + rank)                     # different weights per rank: the start-up broadcast must align them
        opt = _pose_opt(ckpt, gpu_ids=[0, 1], n_gpus_gen=1, ngf=8, n_blocks=2, n_downsample_G=2, n_frames_total=4,
                        max_frames_per_gpu=1, name="roles")
        models = create_model(opt)
        modelG, modelD, flowNet, optimizer_G, optimizer_D, optimizer_D_T = create_optimizer(opt, models)
        L, mD = modelG.layout, modelD.module
        digest = torch.cat([v.detach().double().reshape(-1) for v in mD.netD_f.state_dict().values() if v.numel()]).sum().view(1)
        all_d = [torch.zeros_like(digest) for _ in range(world)]
        dist.all_gather(all_d, digest)
        written = []
        real_save = torch.save
        torch.save = lambda obj, path, *a, **k: (written.append(os.path.basename(path)), real_save(obj, path, *a, **k))
        try:
            mD.save("latest")
        finally:
            torch.save = real_save
        dist.barrier()
        q.put((rank, {"role": L.role, "d_image": L.d_image, "owns_D": L.owns_D, "digests": [float(d) for d in all_d],
                      "written": written, "loss_names": list(mD.loss_names),
                      "in_opt": L.owns_D and {id(p) for p in mD.netD_f.parameters()} <= {id(p) for p in optimizer_D.flat.params}}))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
    finally:
        parallel._ACTIVE_SYNCS.clear()
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.is_available(), reason="dry-run backend: a GPU-less host check")
def test_role_split_keeps_netD_f_on_the_image_discriminator_rank(tmp_path):
    """Two sequence groups of (1 generator + 1 discriminator rank): netD_f lives on D-rank 0 with netD, its state is
    broadcast over the discriminator ranks at start-up, its parameters are in optimizer_D's flat buffer, and D_f is
    written once (by the owner in sequence group 0)."""
    world = 4
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_role_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r, out = q.get(timeout=600)
            res[r] = out
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    for r, out in res.items():
        assert "error" not in out, "rank %d:\n%s" % (r, out.get("error"))
    d_ranks = [r for r, o in res.items() if o["role"] == "D"]
    assert len(d_ranks) == 2 and all(res[r]["owns_D"] and res[r]["in_opt"] for r in d_ranks)
    assert all(res[r]["loss_names"] == LOSS_NAMES for r in res)
    digests = res[0]["digests"]
    assert digests[d_ranks[0]] == digests[d_ranks[1]]
    g_ranks = [r for r in res if r not in d_ranks]
    assert digests[g_ranks[0]] != digests[d_ranks[0]]           # (the generator ranks' unused copies were never aligned)
    writers = [r for r, o in res.items() if "latest_net_D_f.pth" in o["written"]]
    assert len(writers) == 1 and writers[0] in d_ranks
    assert os.path.isfile(os.path.join(str(tmp_path), "roles", "latest_net_D_f.pth"))
