"""The two CPU references of the FlowNet2 backward passes against each other, before any GPU is involved: the reference's own
backward kernel bodies executed on host cores (oracle/ref_ops.py) and torch autograd of the restated forward
(oracle/vid2vid_oracle.py).  tests/test_gpu_flow_bwd.py compares the HIP kernels with both.

Agreement measured here (tests/util.py's metric): resample2d grad_img 3.6e-7, grad_flow 5.1e-7; channelnorm 1.6e-7 (maxima over the cases below)."""
import pytest
import torch

from util import assert_close, rel_err
from flow_bwd_common import away_from_integers, randn, autograd_resample2d, autograd_channelnorm


def _ref_ops():
    from oracle import ref_ops as R
    if not R.available():
        pytest.skip("oracle/_ref/libref_ops.so not built and /root/reference absent")
    return R


@pytest.mark.ref_checker
def test_reference_backward_kernels_agree_with_autograd_of_the_oracle():
    R = _ref_ops()
    for (n, c, h, w, seed) in [(2, 3, 13, 17, 21), (1, 8, 32, 48, 22)]:
        img, flow, go = randn((n, c, h, w), seed), away_from_integers(n, h, w, seed + 50), randn((n, c, h, w), seed + 100)
        ki, kf = R.resample2d_backward(img, flow, go, 1)
        ai, af = autograd_resample2d(img, flow, go, 1)
        print("resample2d grad_img %.3e grad_flow %.3e" % (rel_err(ki, ai), rel_err(kf, af)))
        assert_close(ki, ai, 1e-5, "resample2d grad_img: reference kernel vs autograd")
        assert_close(kf, af, 1e-5, "resample2d grad_flow: reference kernel vs autograd")
    for (n, c, h, w, seed) in [(2, 3, 13, 17, 31), (1, 6, 32, 48, 32)]:
        x, go = randn((n, c, h, w), seed), randn((n, 1, h, w), seed + 1)
        k = R.channelnorm_backward(x, R.channelnorm(x), go)
        a = autograd_channelnorm(x, go)
        print("channelnorm %.3e" % rel_err(k, a))
        assert_close(k, a, 1e-5, "channelnorm backward: reference kernel vs autograd")


def test_flows_keep_away_from_integer_positions():
    flow = away_from_integers(2, 13, 17, 5)
    ys, xs = torch.meshgrid(torch.arange(13.), torch.arange(17.), indexing="ij")
    xf, yf = xs[None] + flow[:, 0], ys[None] + flow[:, 1]
    assert float((xf - xf.round()).abs().min()) >= 1e-3 and float((yf - yf.round()).abs().min()) >= 1e-3
    assert float(xf.min()) < 0 and float(xf.max()) > 16 and float(yf.min()) < 0 and float(yf.max()) > 12      # the clamps bind
