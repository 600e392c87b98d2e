"""Every launch form of the four spatial backward operators (csrc/train_score.hip) against float64 autograd (tests/_spatial_bwd_fp64.py,
pinned without a GPU by tests/test_spatial_bwd_fp64_cpu.py) on the float32 inputs the kernel saw.  The host picks a form by channel count,
alignment, map width and LDS size; nothing reports which one ran, so each test states the dispatch clause its inputs meet (the clauses
were confirmed with one value-only mutant per form, docs/LOG.md).

Arithmetic is held to R.bound (4 x torch's own float32 CPU error against float64, floor 4 ulp of the largest output), computed in each test
from the same inputs.  Pure routing -- the pool where an input belongs to at most one window -- is compared bit for bit.  Every comparison
covers every output element."""
import pytest
import torch

from tests import _leaf_fp64 as R
from tests import _spatial_bwd_fp64 as S

pytestmark = pytest.mark.gpu
SENT = R.SENT


def _ops():
    from vpho_amd import ops
    return ops


def _dev(t, unaligned=False):
    return R.offset_view(t) if unaligned else t.cuda()


# ------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize('k,stride,pad,H,W', [(3, 2, 1, 9, 11), (3, 2, 1, 8, 8), (2, 2, 0, 8, 8), (2, 2, 0, 7, 9)])
@pytest.mark.parametrize('ties', [False, True], ids=['randn', 'ties'])
def test_maxpool_backward_three_forms_agree_bit_for_bit_and_with_torch(k, stride, pad, H, W, ties):
    """two-pass arg-max bytes: ops.maxpool_bwd with k > stride, C % 4 == 0, 16-byte aligned x / dy / dx (with k <= stride the workspace
         size is 0 and the same call takes the one-pass <4> form);
    one-pass maxpool_bwd_kernel<4>: one_pass=True, C % 4 == 0, aligned;
    one-pass maxpool_bwd_kernel<1>: C = 5, or C = 8 with x and dy one element past a 16-byte boundary -- through either entry point.
    k3 s2 p1: overlapping windows cut by all four borders, an input may win up to four windows (a float32 sum: R.bound).  k2 s2 p0: one
    window per input at most, pure routing, bit for bit torch's; on 7x9 the last row and column are in no window.  `ties`: values in
    {0, 1, 2}, a tie in almost every window, the first maximum in row-major order takes the gradient."""
    ops = _ops()
    g = R.gen(H * W + k + ties)
    N = H - 6
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = torch.randint(0, 3, (N, H, W, 8), generator=g).float() if ties else torch.randn(N, H, W, 8, generator=g)
    dy = torch.randn(N, OH, OW, 8, generator=g)
    ref, f32 = S.maxpool_bwd(x.double(), dy.double(), k, stride, pad), S.maxpool_bwd(x, dy, k, stride, pad)
    x5, dy5 = x[..., :5].contiguous(), dy[..., :5].contiguous()                  # the pool is per channel: the reference of the slice is the slice
    two = 'pool two_pass' if k > stride else 'pool one_pass<4>'
    got = [(two, ops.maxpool_bwd(_dev(x), _dev(dy), k, stride, pad), ref),
           ('pool one_pass<4>', ops.maxpool_bwd(_dev(x), _dev(dy), k, stride, pad, one_pass=True), ref),
           ('pool one_pass<1>', ops.maxpool_bwd(_dev(x, True), _dev(dy, True), k, stride, pad, one_pass=True), ref),
           ('pool one_pass<1>', ops.maxpool_bwd(_dev(x, True), _dev(dy, True), k, stride, pad), ref),
           ('pool one_pass<1>', ops.maxpool_bwd(_dev(x5), _dev(dy5), k, stride, pad, one_pass=True), ref[..., :5]),
           ('pool one_pass<1>', ops.maxpool_bwd(_dev(x5), _dev(dy5), k, stride, pad), ref[..., :5])]
    for i, (name, d, r) in enumerate(got):
        if k <= stride:
            assert R.bits_equal(d, r.float()), (name, i)
            assert bool((d[:, OH * stride:] == 0).all()) and bool((d[:, :, OW * stride:] == 0).all())
        else:
            R.check(f'{name} k{k}s{stride}p{pad} {H}x{W} {"ties" if ties else "randn"} #{i}', d, r, R.bound(f32[..., :r.shape[-1]], r))
        assert R.bits_equal(d, got[0][1][..., :d.shape[-1]]), (name, i)          # every form, the same bits
    assert not ties or x.unique().numel() == 3


# ------------------------------------------------------------------------------------------------ bilinear resize
@pytest.mark.parametrize('H,W,OH,OW', [(32, 32, 64, 64), (5, 7, 13, 9), (16, 16, 8, 8), (64, 64, 3, 5), (3, 5, 64, 61), (1, 1, 5, 7), (7, 1, 1, 9)])
@pytest.mark.parametrize('C,unaligned', [(21, False), (8, False), (8, True)], ids=['C21', 'C8', 'C8-unaligned'])
def test_resize_bilinear_backward_both_forms(H, W, OH, OW, C, unaligned):
    """resize_bilinear_bwd_kernel<4>: C % 4 == 0 and dy, dx 16-byte aligned (C = 8);
    resize_bilinear_bwd_kernel<1>: otherwise -- C = 21 (what the training step launches for the hand heat maps), or C = 8 with dy one
    element past a 16-byte boundary.  The production ratio 32 -> 64, odd sizes, both directions, ratios up to 21, single rows / columns.
    A gather in ascending output order: repeated launches give the same bits, and both forms run the same per-channel loop, so the
    unaligned C = 8 launch equals the aligned one bit for bit."""
    ops = _ops()
    N = 1 + (H + OW) % 3
    dy = torch.randn(N, OH, OW, C, generator=R.gen(H * 100 + OW + C))
    ref, tol = R.ruled(S.resize_bilinear_bwd, [dy], H, W)
    form = 'resize<4>' if C % 4 == 0 and not unaligned else 'resize<1>'
    d = _dev(dy, unaligned)
    got = ops.resize_bilinear_bwd(d, H, W)
    R.check(f'{form} N{N} {H}x{W}<-{OH}x{OW} C{C}{" unaligned" if unaligned else ""}', got, ref, tol)
    assert R.bits_equal(ops.resize_bilinear_bwd(d, H, W), got)
    if unaligned:
        assert R.bits_equal(ops.resize_bilinear_bwd(dy.cuda(), H, W), got)


# ------------------------------------------------------------------------------------------------ RoIAlign
FLIP = torch.tensor([1, 0, 1], dtype=torch.uint8)


def _roi_reference(dy, boxes, H, W, P, flip, c_off, C, into):
    """-> float64 reference of into + gradient, its bound, and the float64 gradient alone; the precondition is asserted on the boxes"""
    S.assert_roi_precondition(boxes, H, W, 0.25, P)
    g32 = S.roi_align_bwd(dy, boxes, H, W, 0.25, flip, c_off, C)
    g64 = S.roi_align_bwd(dy.double(), boxes.double(), H, W, 0.25, flip, c_off, C)
    ref = into.double() + g64
    return ref, R.bound(into + g32, ref), g64


def _wide_boxes(H, W):
    """three boxes for the wide maps: the whole map, one leaving it on the left, one on the right, top and bottom"""
    fb = [(0.0, 0.0, float(W), float(H)), (-0.13 * W, 0.15 * H, 0.55 * W, 0.8 * H), (0.47 * W, -0.2 * H, 1.09 * W, 1.35 * H)]
    return torch.tensor([[v / 0.25 for v in b] for b in fb], dtype=torch.float32)


@pytest.mark.parametrize('H,W,P', [(20, 24, 8), (64, 64, 32)])
@pytest.mark.parametrize('group', [0, 1, 2])
@pytest.mark.parametrize('C,ld,c_off', [(8, 8, 0), (8, 16, 4)], ids=['whole', 'slice'])
def test_roi_align_backward_gather_form(H, W, P, group, C, ld, c_off):
    """roi_align_bwd_gather_kernel: C % 4 == 0, ldo % 4 == 0, c_off % 4 == 0, dy and dfeat 16-byte aligned, W <= 192, P <= 256 and
    (P + W P) floats + (2 + 2 W) ints of LDS <= 48 KB.  A non-square 20x24 map with P = 8 and the production geometry 64x64 with P = 32;
    the nine box kinds of S.roi_boxes three at a time, flip on images 0 and 2; the gradient slice c_off 4 of ldo 16; accumulation
    into a gradient pre-filled with 7.0 -- where the float64 gradient is exactly 0 (outside every sample's four taps) the 7.0 must
    survive bit for bit.  Fixed summation order: three launches, the same bits."""
    ops = _ops()
    g = R.gen(H + P + group + c_off)
    boxes = S.roi_boxes(H, W, 0.25, P)[3 * group:3 * group + 3]
    dy = torch.randn(3, P, P, ld, generator=g)
    into = torch.full((3, H, W, C), 7.0)
    ref, tol, g64 = _roi_reference(dy, boxes, H, W, P, FLIP, c_off, C, into)
    run = lambda: ops.roi_align_bwd(dy.cuda(), boxes.cuda(), (H, W), C, 0.25, flip_w=FLIP.cuda(), c_off=c_off, into=into.cuda())
    got = run()
    R.check(f'roi gather {H}x{W} P{P} {"/".join(S.ROI_KINDS[3 * group:3 * group + 3])} c_off{c_off} ldo{ld}', got, ref, tol)
    zero = g64 == 0
    assert bool(zero.any()) and R.bits_equal(got.cpu()[zero], torch.full((int(zero.sum()),), 7.0))
    if group == 1:
        assert bool(zero[2].all())                                               # the box entirely outside the map
    for _ in range(2):
        assert R.bits_equal(run(), got)


def test_roi_align_backward_gather_form_at_its_widest_map():
    """roi_align_bwd_gather_kernel at W = 192, the widest map it takes (threads 64 .. 255 each find one column's bin range): P = 4,
    H = 2, C = 8, LDS 4 624 B.  The whole-map box has 48 samples per bin along x."""
    ops = _ops()
    H, W, P, C = 2, 192, 4, 8
    boxes = _wide_boxes(H, W)
    dy = torch.randn(3, P, P, C, generator=R.gen(192))
    into = torch.full((3, H, W, C), 7.0)
    ref, tol, g64 = _roi_reference(dy, boxes, H, W, P, FLIP, 0, C, into)
    run = lambda: ops.roi_align_bwd(dy.cuda(), boxes.cuda(), (H, W), C, 0.25, flip_w=FLIP.cuda(), into=into.cuda())
    got = run()
    R.check('roi gather 2x192 P4 widest', got, ref, tol)
    zero = g64 == 0
    assert bool(zero.any()) and R.bits_equal(got.cpu()[zero], torch.full((int(zero.sum()),), 7.0))
    for _ in range(2):
        assert R.bits_equal(run(), got)


ROI_ATOMIC = {  # the clause of the dispatch that sends the call to roi_align_bwd_kernel: H, W, P, C, ldo, c_off, dy unaligned
    'C6': (20, 24, 8, 6, 6, 0, False),                      # C % 4 != 0
    'c_off3-ldo13': (20, 24, 8, 8, 13, 3, False),           # c_off % 4 != 0 and ldo % 4 != 0
    'dy-unaligned': (20, 24, 8, 8, 8, 0, True),             # dy not 16-byte aligned
    'W193': (2, 193, 4, 4, 4, 0, False),                    # W > 192
    'W192-P64': (64, 192, 64, 4, 4, 0, False),              # (64 + 192 * 64) * 4 + (2 + 384) * 4 = 50 952 B of LDS > 48 KB
}
# The height of the P = 64 case is 64, not 2: the bound's factor 4 allows for another summation ORDER of sums as long as torch's.  On two
# rows all 64 bin rows of a box fold onto the same pixels, each output becomes an unordered float32 sum of well over a hundred atomic adds,
# and its rounding grows with that length, not with anything the kernel computes (measured so: 8.7e-6 against 7.7e-6, docs/LOG.md).  With
# bins one pixel high an output collects a dozen terms, as in the training step (two-pixel bins, 2 x 2 samples).


@pytest.mark.parametrize('clause', list(ROI_ATOMIC))
@pytest.mark.parametrize('group', [0, 1, 2])
def test_roi_align_backward_atomic_form(clause, group):
    """roi_align_bwd_kernel (fp32 atomics), reached once through each clause of the dispatch that refuses the gather form (ROI_ATOMIC).
    Two launches as in the training step: a first set of boxes into zeros, then a second set, flipped on images 0 and 2, accumulated with
    into= (atomics round at every add into the destination, so the accumulated-into values are gradients, not a large constant).  With dy
    unaligned the same values also go through the gather form (aligned copy): the two results agree within the sum of their bounds."""
    ops = _ops()
    H, W, P, C, ld, c_off, unaligned = ROI_ATOMIC[clause]
    if W > 64:
        a = _wide_boxes(H, W)
        a, b = a[[group, (group + 1) % 3, (group + 2) % 3]], a[[(group + 1) % 3, (group + 2) % 3, group]] * 0.8 + 0.9
    else:
        nine = S.roi_boxes(H, W, 0.25, P)
        a, b = nine[3 * group:3 * group + 3], nine[[(3 * group + 4) % 9, (3 * group + 8) % 9, (3 * group + 6) % 9]]
    g = R.gen(W + P + C + group)
    dy1, dy2 = torch.randn(3, P, P, ld, generator=g), torch.randn(3, P, P, ld, generator=g)
    for bx in (a, b):
        S.assert_roi_precondition(bx, H, W, 0.25, P)

    def both(d1, d2, ba, bb):                                                    # in the dtype of its arguments
        return S.roi_align_bwd(d2, bb, H, W, 0.25, FLIP, c_off, C, into=S.roi_align_bwd(d1, ba, H, W, 0.25, None, c_off, C))

    def run(un):
        df = ops.roi_align_bwd(_dev(dy1, un), a.cuda(), (H, W), C, 0.25, c_off=c_off)
        return ops.roi_align_bwd(_dev(dy2, un), b.cuda(), (H, W), C, 0.25, flip_w=FLIP.cuda(), c_off=c_off, into=df)

    ref, tol = R.ruled(both, [dy1, dy2, a, b])
    got = run(unaligned)
    R.check(f'roi atomic {clause} {H}x{W} P{P} group{group}', got, ref, tol)
    if unaligned:
        gather = run(False)
        R.check(f'roi gather {H}x{W} P{P} group{group} (aligned twin of {clause})', gather, ref, tol)
        assert R.worst(got, gather.cpu()) <= 2 * tol


# ------------------------------------------------------------------------------------------------ heat-map re-alignment
def _align_case(S_, C, kind):
    g = R.gen(S_ * 10 + C)
    bbox, rect = R.boxes(3, g, kind)
    dout = torch.randn(3, S_, S_, C, generator=g)
    ref, tol = R.ruled(S.align_heatmap_bwd, [dout, bbox, rect], FLIP)
    return dout, bbox, rect, ref, tol


@pytest.mark.parametrize('S_,C', [(64, 21), (16, 5), (122, 1)])
@pytest.mark.parametrize('kind', ['equal', 'larger', 'smaller'])
def test_align_heatmap_backward_gather_form(S_, C, kind):
    """align_heatmap_bwd_gather_kernel: S <= 192 and (S + S S) floats + (2 + 2 S) ints of LDS <= 60 KB, i.e. S <= 122.  S = 64 with
    C = 21 is what the training step launches; S = 122 is the largest launch of this form (61 008 B of dynamic LDS).  Rectangles equal
    to, larger than (samples outside the map: zero padding) and smaller than the box; flip on images 0 and 2.  Fixed summation order:
    three launches, the same bits."""
    ops = _ops()
    dout, bbox, rect, ref, tol = _align_case(S_, C, kind)
    run = lambda: ops.align_heatmap_bwd(dout.cuda(), bbox.cuda(), rect.cuda(), FLIP.cuda())
    got = run()
    R.check(f'hm gather S{S_} C{C} {kind}', got, ref, tol)
    for _ in range(2):
        assert R.bits_equal(run(), got)


@pytest.mark.parametrize('S_', [123, 128])
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('kind', ['equal', 'larger', 'smaller'])
def test_align_heatmap_backward_atomic_form(S_, C, kind):
    """align_heatmap_bwd_kernel (fp32 atomics): S >= 123, where the gather form's tables no longer fit 60 KB of LDS"""
    ops = _ops()
    dout, bbox, rect, ref, tol = _align_case(S_, C, kind)
    got = ops.align_heatmap_bwd(dout.cuda(), bbox.cuda(), rect.cuda(), FLIP.cuda())
    R.check(f'hm atomic S{S_} C{C} {kind}', got, ref, tol)


# ------------------------------------------------------------------------------------------------ guards
def test_argument_guards_raise_and_launch_nothing():
    """size <= 1 (heat-map alignment), ldo < c_off + C and c_off < 0 (RoIAlign) answer VphoError before anything is launched: the
    destination keeps its sentinel.  The buffers passed are valid for the sizes the call names."""
    ops = _ops()
    dev = 'cuda'
    box = torch.tensor([[0.0, 0.0, 10.0, 10.0]] * 2, device=dev)
    dhm = torch.full((2, 1, 1, 3), SENT, device=dev)
    with pytest.raises(ops.VphoError):
        ops.align_heatmap_bwd(torch.zeros(2, 1, 1, 3, device=dev), box, box)     # size <= 1 through the wrapper
    with pytest.raises(ops.VphoError):                                           # and with a destination of our own to look at
        ops._call('vpho_align_heatmap_bwd_nhwc_f32', torch.zeros(2, 1, 1, 3, device=dev), 2, 1, 3, box, box,
                  None, dhm)
    df = torch.full((2, 4, 4, 8), SENT, device=dev)
    dy = torch.zeros(2, 2, 2, 8, device=dev)
    with pytest.raises(ops.VphoError):
        ops.roi_align_bwd(dy, box, (4, 4), 8, 0.25, c_off=4, into=df)            # ldo < c_off + C
    with pytest.raises(ops.VphoError):
        ops.roi_align_bwd(dy, box, (4, 4), 4, 0.25, c_off=-4, into=df)           # c_off < 0
    torch.cuda.synchronize()
    assert bool((dhm == SENT).all()) and bool((df == SENT).all())
