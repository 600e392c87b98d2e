"""Autograd references of the four spatial backward operators of the training step (csrc/train_score.hip: max-pool, bilinear resize,
RoIAlign, heat-map re-alignment).  TEST INFRASTRUCTURE ONLY: plain torch and the CPU oracle, nothing here imports ``vpho_amd.ops``.

As in tests/_leaf_fp64.py every function computes in the dtype of its tensor arguments, so ``R.ruled(f, args, ...)`` gives the float64
reference (autograd in float64 on the float32 inputs) and, from torch's own float32 evaluation of the same graph, the bound.  Maps are
NHWC.  What a forward computes in float32 whatever its input (the RoI geometry of oracle.roi_align, the base grid of
oracle.vpho.align_hm_to_bbox_rectangle) stays float32 in both evaluations: it selects taps and grid counts, it is not rounding noise."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.roi_align import roi_align_fast
from oracle.vpho import align_hm_to_bbox_rectangle, flip_w


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def maxpool_bwd(x, dy, k, stride, pad):
    """x (N,H,W,C), dy (N,OH,OW,C) -> d x of F.max_pool2d (ties: the first maximum in row-major window order)"""
    xx = _nchw(x).detach().requires_grad_(True)
    return _nhwc(torch.autograd.grad(F.max_pool2d(xx, k, stride, pad), xx, _nchw(dy))[0])


def resize_bilinear_bwd(dy, H, W):
    """dy (N,OH,OW,C) -> d x (N,H,W,C) of F.interpolate(x, (OH, OW), mode='bilinear', align_corners=False)"""
    N, OH, OW, C = dy.shape
    x = dy.new_zeros((N, C, H, W)).requires_grad_(True)
    y = F.interpolate(x, size=(OH, OW), mode='bilinear', align_corners=False)
    return _nhwc(torch.autograd.grad(y, x, _nchw(dy))[0])


def roi_align_bwd(dy, boxes, H, W, scale, flip=None, c_off=0, C=None, into=None):
    """dy (N,P,P,ld), its channels c_off .. c_off+C the gradient of roi_align(feat, one box per image, (P, P), scale) -- flipped along
    the bin columns where `flip` -- -> d feat (N,H,W,C), added to `into` if given"""
    N, P, _, ld = dy.shape
    C = ld - c_off if C is None else C
    feat = dy.new_zeros((N, C, H, W)).requires_grad_(True)
    rois = torch.cat([torch.arange(N, dtype=boxes.dtype)[:, None], boxes], 1)
    y = roi_align_fast(feat, rois, P, scale)
    if flip is not None:
        y = flip_w(y, flip.bool())
    g = _nhwc(torch.autograd.grad(y, feat, _nchw(dy[..., c_off:c_off + C]))[0])
    return g if into is None else into + g


def align_heatmap_bwd(dout, bbox, rect, flip=None):
    """dout (N,S,S,C) -> d hm (N,S,S,C) of flip_w(align_hm_to_bbox_rectangle(hm, bbox, rect, S), flip)"""
    N, S, _, C = dout.shape
    hm = dout.new_zeros((N, C, S, S)).requires_grad_(True)
    y = align_hm_to_bbox_rectangle(hm, bbox, rect, S)
    if flip is not None:
        y = flip_w(y, flip.bool())
    return _nhwc(torch.autograd.grad(y, hm, _nchw(dout))[0])


# ------------------------------------------------------------------------------------------------ RoI boxes and their precondition
_f = np.float32


def roi_samples(box, scale, P):
    """float32 geometry of one RoI as torchvision's float kernel computes it: grid counts (gh, gw) and the sample coordinates ys, xs"""
    x1, y1, x2, y2 = (_f(_f(v) * _f(scale)) for v in box)
    rw, rh = max(_f(x2 - x1), _f(1.0)), max(_f(y2 - y1), _f(1.0))
    bh, bw = _f(rh / _f(P)), _f(rw / _f(P))
    gh, gw = int(math.ceil(bh)), int(math.ceil(bw))
    ax = lambda o, b, g: [_f(_f(o + _f(_f(p) * b)) + _f(_f(_f(i + 0.5) * b) / _f(g))) for p in range(P) for i in range(g)]
    return gh, gw, ax(y1, bh, gh), ax(x1, bw, gw)


def assert_roi_precondition(boxes, H, W, scale, P):
    """The forward is discontinuous only where a grid count ceil(roi / P) steps and where a sample crosses -1 or H (W).  A test box must sit
    away from both, or float32 and float64 would legitimately differ: the counts agree in both precisions and no sample coordinate lies
    within 1e-3 of -1 or of the map's size.  Judged from the boxes alone; a violation is a bad test input."""
    for box in boxes.tolist():
        gh, gw, ys, xs = roi_samples(box, scale, P)
        x1, y1, x2, y2 = (float(_f(v)) * float(_f(scale)) for v in box)
        assert gh == int(math.ceil(max(y2 - y1, 1.0) / P)) and gw == int(math.ceil(max(x2 - x1, 1.0) / P)), (box, gh, gw)
        for coords, L in ((ys, H), (xs, W)):
            for s in coords:
                assert abs(float(s) + 1.0) > 1e-3 and abs(float(s) - L) > 1e-3, (box, float(s), L)


def roi_boxes(H, W, scale, P):
    """nine boxes in image coordinates for an (H, W) map, one per kind (names in ROI_KINDS)"""
    ix, iy = round(0.125 * W) + 0.5, round(0.1 * H) + 0.25            # exact in float32, as is the size: P * (whole number of pixels per bin)
    iw, ih = P * max(1, int(0.7 * W) // P), P * max(1, int(0.7 * H) // P)
    fb = [(0.14 * W, 0.11 * H, 0.73 * W, 0.77 * H),                    # interior
          (-0.16 * W, 0.21 * H, 0.41 * W, 0.83 * H),                   # left edge outside
          (0.22 * W, -0.19 * H, 0.87 * W, 0.52 * H),                   # top edge outside
          (0.55 * W, 0.13 * H, 1.17 * W, 0.69 * H),                    # right edge outside
          (0.09 * W, 0.47 * H, 0.66 * W, 1.21 * H),                    # bottom edge outside
          (W + 5.3, 0.2 * H, W + 12.9, 0.7 * H),                       # entirely outside: every sample has x > W, gradient exactly 0
          (0.4 * W + 0.3, 0.15 * H, 0.4 * W + 0.7, 0.8 * H),           # narrower than one feature pixel: width clamped to 1
          (ix, iy, ix + iw, iy + ih),                                  # bin size an exact integer: ceil() sits on its step
          (0.0, 0.0, float(W), float(H))]                              # the whole map
    return torch.tensor([[v / scale for v in b] for b in fb], dtype=torch.float32)


ROI_KINDS = ('interior', 'left', 'top', 'right', 'bottom', 'outside', 'narrow', 'integer_bin', 'whole')
