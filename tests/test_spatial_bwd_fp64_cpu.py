"""The autograd references of tests/_spatial_bwd_fp64.py held to a second formulation written out here -- a dense adjoint matrix built from
the forward's sampling rule (resize, RoIAlign, heat-map alignment), an explicit arg-max scatter (pool) -- at the smallest shapes, in
float64, to 1e-12 of the output scale: a wrong reference must not be what tests/test_gpu_spatial_bwd.py measures the kernels with.  No GPU."""
import math

import numpy as np
import pytest
import torch

from tests import _leaf_fp64 as R
from tests import _spatial_bwd_fp64 as S

f64 = torch.float64


def _close(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == f64
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------ max-pool
def _pool_scatter(x, dy, k, stride, pad):
    """every window hands its dy to its first maximum in row-major order"""
    N, H, W, C = x.shape
    dx = torch.zeros_like(x)
    for n in range(N):
        for c in range(C):
            for oy in range(dy.shape[1]):
                for ox in range(dy.shape[2]):
                    best = None
                    for r in range(k):
                        for q in range(k):
                            yy, xx = oy * stride - pad + r, ox * stride - pad + q
                            if 0 <= yy < H and 0 <= xx < W and (best is None or float(x[n, yy, xx, c]) > float(x[n, best[0], best[1], c])):
                                best = (yy, xx)
                    dx[n, best[0], best[1], c] += dy[n, oy, ox, c]
    return dx


@pytest.mark.parametrize('H,W,k,stride,pad', [(9, 11, 3, 2, 1), (8, 8, 3, 2, 1), (8, 8, 2, 2, 0), (7, 9, 2, 2, 0)])
@pytest.mark.parametrize('ties', [False, True])
def test_pool_reference_is_the_first_maximum_scatter(H, W, k, stride, pad, ties):
    g = R.gen(H * W + k)
    x = torch.randint(0, 3, (2, H, W, 3), generator=g).to(f64) if ties else torch.randn(2, H, W, 3, generator=g, dtype=f64)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = torch.randn(2, OH, OW, 3, generator=g, dtype=f64)
    got = S.maxpool_bwd(x, dy, k, stride, pad)
    _close(got, _pool_scatter(x, dy, k, stride, pad))
    if k <= stride:
        assert bool((got[:, OH * stride:] == 0).all()) and bool((got[:, :, OW * stride:] == 0).all())      # rows / columns in no window


def test_pool_tie_rule_on_the_all_zero_map():
    """all-zero 4x4, k3 s2 p1, dy = 1..4: the gradient lands on (0,0), (0,1), (1,0), (1,1) -- the first in-map element of each window"""
    x, dy = torch.zeros(1, 4, 4, 1, dtype=f64), torch.arange(1.0, 5.0, dtype=f64).view(1, 2, 2, 1)
    want = torch.zeros(1, 4, 4, 1, dtype=f64)
    want[0, 0, 0, 0], want[0, 0, 1, 0], want[0, 1, 0, 0], want[0, 1, 1, 0] = 1, 2, 3, 4
    assert torch.equal(S.maxpool_bwd(x, dy, 3, 2, 1), want)


# ------------------------------------------------------------------------------------------------ bilinear resize
def _resize_axis(n_in, n_out):
    """(n_out, n_in): s = max((o + 0.5) n_in / n_out - 0.5, 0), taps floor(s) and min(floor(s) + 1, n_in - 1)"""
    A = torch.zeros(n_out, n_in, dtype=f64)
    for o in range(n_out):
        s = max((o + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = int(s)
        i1 = min(i0 + 1, n_in - 1)
        A[o, i0] += 1.0 - (s - i0)
        A[o, i1] += s - i0
    return A


@pytest.mark.parametrize('H,W,OH,OW', [(5, 7, 13, 9), (16, 16, 8, 8), (8, 8, 3, 5), (3, 5, 16, 13), (1, 1, 5, 7), (7, 1, 1, 9)])
def test_resize_reference_is_the_transposed_sampling_matrix(H, W, OH, OW):
    dy = torch.randn(2, OH, OW, 3, generator=R.gen(H * OW), dtype=f64)
    M = torch.kron(_resize_axis(H, OH), _resize_axis(W, OW))                      # (OH*OW, H*W): out = M x
    want = torch.einsum('op,noc->npc', M, dy.reshape(2, OH * OW, 3)).reshape(2, H, W, 3)
    _close(S.resize_bilinear_bwd(dy, H, W), want)
    assert float((M.sum(1) - 1).abs().max()) < 1e-14                              # every output is a convex combination


# ------------------------------------------------------------------------------------------------ RoIAlign
def _roi_matrix(box, H, W, scale, P):
    """(P*P, H*W) of one RoI: float32 sample coordinates and float32 bilinear weights (torchvision's float kernel), summed in float64"""
    gh, gw, ys, xs = S.roi_samples(box, scale, P)
    f = np.float32

    def taps(s, L):
        if s < -1.0 or s > L:
            return None
        s = max(s, f(0.0))
        lo = int(s)
        if lo >= L - 1:
            lo = hi = L - 1
            s = f(lo)
        else:
            hi = lo + 1
        l = f(s - f(lo))
        return lo, hi, l, f(f(1.0) - l)

    M = torch.zeros(P * P, H * W, dtype=f64)
    for ph in range(P):
        for pw in range(P):
            for y in ys[ph * gh:(ph + 1) * gh]:
                for x in xs[pw * gw:(pw + 1) * gw]:
                    ty, tx = taps(y, H), taps(x, W)
                    if ty is None or tx is None:
                        continue
                    (yl, yh, ly, hy), (xl, xh, lx, hx) = ty, tx
                    for yy, xx, w in ((yl, xl, f(hy * hx)), (yl, xh, f(hy * lx)), (yh, xl, f(ly * hx)), (yh, xh, f(ly * lx))):
                        M[ph * P + pw, yy * W + xx] += float(w)
    return M / max(gh * gw, 1)


@pytest.mark.parametrize('group', [0, 1, 2])
def test_roi_align_reference_is_the_transposed_sampling_matrix(group):
    H, W, P, C, scale = 20, 24, 8, 3, 0.25
    g = R.gen(group)
    boxes = S.roi_boxes(H, W, scale, P)[3 * group:3 * group + 3]
    S.assert_roi_precondition(boxes, H, W, scale, P)
    flip = torch.tensor([1, 0, 1], dtype=torch.uint8)
    dy = torch.randn(3, P, P, C + 3, generator=g, dtype=f64)
    into = torch.randn(3, H, W, C, generator=g, dtype=f64)
    want = into.clone()
    for n in range(3):
        d = dy[n, :, :, 2:2 + C]
        d = d.flip(1) if flip[n] else d                                          # the forward's output was flipped along the bin columns
        want[n] += (_roi_matrix(boxes[n].tolist(), H, W, scale, P).t() @ d.reshape(P * P, C)).reshape(H, W, C)
    _close(S.roi_align_bwd(dy, boxes.double(), H, W, scale, flip, 2, C, into), want)
    if group == 1:
        assert S.ROI_KINDS[5] == 'outside' and torch.equal(want[2], into[2])     # entirely outside: nothing arrives


def test_roi_boxes_cover_their_kinds_and_meet_the_precondition():
    """what each kind is for holds by the float32 geometry, at both geometries of the GPU tests; and the precondition does reject a box
    whose grid count differs between float32 and float64 or whose samples touch a discontinuity"""
    for H, W, P in ((20, 24, 8), (64, 64, 32)):
        boxes = S.roi_boxes(H, W, 0.25, P)
        S.assert_roi_precondition(boxes, H, W, 0.25, P)
        geo = dict(zip(S.ROI_KINDS, (S.roi_samples(b, 0.25, P) for b in boxes.tolist())))
        inside = lambda s, L: -1.0 <= s <= L
        assert all(inside(s, H) for s in geo['interior'][2]) and all(inside(s, W) for s in geo['interior'][3])
        assert min(geo['left'][3]) < -1 and min(geo['top'][2]) < -1 and max(geo['right'][3]) > W and max(geo['bottom'][2]) > H
        assert all(s > W for s in geo['outside'][3])
        assert geo['narrow'][1] == 1 and abs((geo['narrow'][3][-1] - geo['narrow'][3][0]) - (P - 1) / P) < 1e-5    # width clamped to 1: bins of 1 / P
        b = boxes[7].tolist()
        assert ((b[2] - b[0]) * 0.25 / P).is_integer() and ((b[3] - b[1]) * 0.25 / P).is_integer()
        assert geo['whole'][0] == math.ceil(H / P) and geo['whole'][1] == math.ceil(W / P)
    with pytest.raises(AssertionError):                                          # width 64 + 2^-20: 64 in float32 (grid count 2), count 3 in float64
        S.assert_roi_precondition(torch.tensor([[2.0 ** -15 - 2.0 ** -18, 0.0, 256.0 + 2.0 ** -15, 100.0]]), 64, 64, 0.25, 32)
    with pytest.raises(AssertionError):                                          # bins of 0.5 from x = -1.25: the first sample sits on -1 exactly
        S.assert_roi_precondition(torch.tensor([[-5.0, 0.0, 11.0, 64.0]]), 20, 24, 0.25, 8)


# ------------------------------------------------------------------------------------------------ heat-map re-alignment
def _align_axis(S_, rel):
    """(S sample, S position): sample k sits at ((lin[k] rel + 1) S - 1) / 2, lin the float32 base grid of the reference code; zeros outside"""
    lin = (torch.arange(S_) / (S_ - 1) * 2 - 1).to(f64)
    B = torch.zeros(S_, S_, dtype=f64)
    for k in range(S_):
        t = ((float(lin[k]) * rel + 1.0) * S_ - 1.0) / 2.0
        p0 = math.floor(t)
        for p, w in ((p0, 1.0 - (t - p0)), (p0 + 1, t - p0)):
            if 0 <= p < S_:
                B[k, p] += w
    return B


@pytest.mark.parametrize('S_,C', [(16, 3), (7, 2)])
@pytest.mark.parametrize('kind', ['equal', 'larger', 'smaller'])
def test_align_heatmap_reference_is_the_transposed_sampling_matrix(S_, C, kind):
    g = R.gen(S_ + C)
    N = 3
    bbox, rect = R.boxes(N, g, kind, f64)
    flip = torch.tensor([1, 0, 1], dtype=torch.uint8)
    dout = torch.randn(N, S_, S_, C, generator=g, dtype=f64)
    want = torch.zeros(N, S_, S_, C, dtype=f64)
    for n in range(N):
        relw = float((rect[n, 2] - rect[n, 0]) / (bbox[n, 2] - bbox[n, 0]))
        relh = float((rect[n, 3] - rect[n, 1]) / (bbox[n, 3] - bbox[n, 1]))
        Bx, By = _align_axis(S_, relw), _align_axis(S_, relh)                     # output index i walks x, j walks y (the axis swap)
        d = dout[n].flip(1) if flip[n] else dout[n]
        want[n] = torch.einsum('ix,jy,ijc->yxc', Bx, By, d)
    _close(S.align_heatmap_bwd(dout, bbox, rect, flip), want)
    # the adjoint of the forward reference of tests/_leaf_fp64.py as well: <A hm, dout> = <hm, A^T dout> (that one builds its grid in float64)
    hm = torch.randn(N, S_, S_, C, generator=g, dtype=f64)
    lhs, rhs = float((R.align_heatmap_gather(hm, bbox, rect, flip) * dout).sum()), float((hm * want).sum())
    assert abs(lhs - rhs) < 1e-5 * float(dout.abs().sum())
