"""Flat option namespace with the reference's defaults for the hot-path flags.

The reference's argparse front end (options/base_options.py:11-85, train_options.py:5-43,
test_options.py:5-15) is kept verbatim by a drop-in user; this helper only builds the same
namespace programmatically for tests, bench.py and smoke() -- names, defaults and the
post-processing of `parse()` (base_options.py:96-109) are the reference's.
"""
from types import SimpleNamespace

_DEFAULTS = dict(
    # base_options.py
    dataroot="datasets/Cityscapes/", batchSize=1, loadSize=512, fineSize=512, input_nc=3, label_nc=0, output_nc=3,
    netG="composite", ngf=128, ndf=64, n_blocks=9, n_downsample_G=3, gpu_ids=[0], n_gpus_gen=-1,
    name="experiment_name", dataset_mode="temporal", model="vid2vid", checkpoints_dir="./checkpoints", norm="batch",
    use_instance=False, label_feat=False, feat_num=3, n_blocks_local=3, n_local_enhancers=1,
    n_frames_G=3, n_scales_spatial=1, no_first_img=False, use_single_G=False, fg=False, fg_labels=[26], no_flow=False,
    openpose_only=False, densepose_only=False, add_face_disc=False, load_pretrain="", debug=False, fp16=False,
    local_rank=0,
    # test_options.py
    which_epoch="latest", use_real_img=False, how_many=300,
    # train_options.py
    isTrain=False, continue_train=False, niter=10, niter_decay=10, beta1=0.5, lr=0.0002, TTUR=False,
    gan_mode="ls", num_D=2, pool_size=1, n_layers_D=3, no_vgg=False, no_ganFeat=False, lambda_feat=10.0, lambda_F=10.0,
    lambda_T=10.0, sparse_D=False, n_scales_temporal=2, n_frames_D=3, n_frames_total=30, max_frames_per_gpu=1,
    max_frames_backpropagate=1, max_t_step=1, niter_step=5, niter_fix_global=0,
    # vid2vid_amd additions
    precision=None,           # 'fp32' | 'bf16' | None (None: bf16 iff opt.fp16)
    random_init_ok=False,     # allow create_model() without a G0 checkpoint (benchmarks / smoke)
    vgg19_checkpoint="checkpoints/vgg19-dcbb9e9d.pth",   # torchvision's vgg19 state_dict (the reference downloads it)
    fix_update_fixed_params=False,   # True: update_fixed_params rebuilds the captured optimizer over all scales (the reference's
                                     # evident intent); False: the reference's observable behaviour (models/base_model.py docstring)
    compact_streams=False,    # multi-stream inference replays a plan with one row per ACTIVE stream (stream pool)
    frames_u8=False,          # inference returns uint8 (B,H,W,3) images written by the frame plan's last launch instead of the fp32
                              # fake_B planes; an idle stream's image is zero bytes; read per call
    inputs_u8=False,          # label_nc == 0 models: input_A is uint8 HWC (B,t,H,W,in_ch), the whole window (t = n_frames_G) on the first
                              # call of a sequence, afterwards the newest frame alone (t = 1); decoded by the frame plan's first
                              # launch through opt.input_lut; read per call
    inputs_u8_slots=False,    # with inputs_u8: restart= / active= and compact_streams take uint8 inputs too -- the slot plan and the
                              # stream pool own uint8 input windows, decoded under the plan's words; read per call
    real_A_u8=False,          # inference's second result is the uint8 input picture (B,H,W,3) -- visual.tensor2label of real_A_last, written
                              # by one launch of the frame plan from the label map itself; tensor2im(normalize=False) of its first
                              # plane(s) for label_nc == 0 -- instead of the fp32 planes; read per call
    input_geometry=None,      # with inputs_u8: input_A is uint8 (B,t,Hs,Ws,in_ch) at SOURCE size, and this is the reference's
                              # get_img_params dict (new_size, crop_size, crop_pos, flip), or a list of B of them: one launch in front
                              # of the frame plan does the loader's nearest resize, crop and flip into the plan's uint8 windows
                              # (DESIGN 3.24); None: input_A is at model size, as before; read per call
    input_lut=None,           # fp32 (in_ch, 256): decoded value of every byte per channel; None = visual.input_lut(in_ch)
    ema_decay=0.0,           # training: > 0 keeps an exponential moving average of the generator's weights inside the Adam step
                              # and saves it as '<label>_net_G<s>_ema.pth' (DESIGN 3.17); 0 = off, nothing changes
    use_ema=False,            # inference: load '<epoch>_net_G<s>_ema.pth' instead of '<epoch>_net_G<s>.pth'
    max_grad_norm=0.0,        # training: > 0 clips every optimizer's gradient to this global L2 norm (torch.nn.utils.clip_grad_norm_'s
                              # rule) on the device, inside the Adam step; 0 = off, nothing changes
    skip_nonfinite_grads=False,   # training: an optimizer step whose gradient holds an inf or a NaN is skipped -- weights, moments, the
                              # averaged weights and the step count stay as they were; model.grad_guard_stats() reports
)


def make_opt(**overrides):
    d = dict(_DEFAULTS)
    unknown = set(overrides) - set(d)
    if unknown:
        raise KeyError("unknown option(s): %s" % sorted(unknown))
    d.update(overrides)
    opt = SimpleNamespace(**d)
    if isinstance(opt.fg_labels, str):
        opt.fg_labels = [int(s) for s in opt.fg_labels.split(",") if int(s) >= 0]
    if isinstance(opt.gpu_ids, str):
        opt.gpu_ids = [int(s) for s in opt.gpu_ids.split(",") if int(s) >= 0]
    if opt.n_gpus_gen == -1:
        opt.n_gpus_gen = len(opt.gpu_ids)
    return opt
