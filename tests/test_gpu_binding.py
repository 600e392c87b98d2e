"""The typed binding (vpho_amd/abi.py) on the device, through three public wrappers at 1 x 4 x 4 x 4: an argument the header does not
declare -- a float64 tensor for `const float*`, an int64 index tensor for `const int*`, a non-contiguous slice -- is refused while the
arguments are converted, so the entry point is never entered and the destination keeps its bits; with the declared types the same
wrappers give what they gave before the binding was typed (the float64 references of tests/_leaf_fp64.py: bit for bit for the two
data-movement kernels, R.ruled's bound for the interpolation)."""
import pytest
import torch

from tests import _leaf_fp64 as R

pytestmark = pytest.mark.gpu
SENT = R.SENT


def _ops():
    from vpho_amd import ops
    return ops


@pytest.fixture
def destination(monkeypatch):
    """the wrappers below allocate their result with ops._new: hand them buffers we keep, filled with a sentinel"""
    ops = _ops()
    made = []

    def new(shape, like, dtype=torch.float32):
        made.append(torch.full(tuple(shape), SENT, device=like.device, dtype=dtype))
        return made[-1]
    monkeypatch.setattr(ops, '_new', new)
    return made


def _untouched(buffers):
    torch.cuda.synchronize()
    return all(bool((b == SENT).all()) for b in buffers)


def test_a_float64_tensor_for_a_float_pointer_is_refused_before_the_launch(destination):
    ops = _ops()
    x = torch.randn(1, 4, 4, 4, generator=R.gen(1))
    with pytest.raises(ops.VphoError, match=r'expected torch\.float32, got torch\.float64'):
        ops.maxpool_nhwc(x.double().cuda(), 2, 2, 0)
    assert len(destination) == 1 and destination[0].shape == (1, 2, 2, 4) and _untouched(destination)
    got = ops.maxpool_nhwc(x.cuda(), 2, 2, 0)
    assert got is destination[1] and R.bits_equal(got, R.maxpool_nhwc(x.double(), 2, 2, 0).float())


def test_an_int64_index_tensor_for_an_int_pointer_is_refused_before_the_launch():
    ops = _ops()
    N, H, W, C, OH, OW = 1, 2, 2, 4, 4, 4
    x = torch.randn(N, H, W, C, generator=R.gen(2))
    win = ops.roi_windows(torch.tensor([[2.0, 2.0, 10.0, 12.0]]).cuda(), None, N, OH, OW, 0.25)
    n = int(win.count.item())
    assert 0 < n <= N * OH * OW
    out = torch.full((N, OH, OW, C), SENT, device='cuda')
    wide = ops.RoiWindows(win.wins, win.row_map.long(), win.count, win.shape)
    with pytest.raises(ops.VphoError, match=r'expected torch\.int32, got torch\.int64'):
        ops.resize_bilinear_nhwc(x.cuda(), OH, OW, out=out, rows=wide)
    assert _untouched([out])
    ops.resize_bilinear_nhwc(x.cuda(), OH, OW, out=out, rows=win)
    listed = torch.zeros(N * OH * OW, dtype=torch.bool)
    listed[win.row_map[:n].long().cpu()] = True
    listed = listed.view(N, OH, OW)
    ref, tol = R.ruled(R.resize_bilinear_nhwc, [x], OH, OW)
    o = out.cpu()
    assert bool((o[~listed] == SENT).all())
    R.check('resize_bilinear rows 1x4x4x4', o[listed], ref[listed], tol)


def test_a_non_contiguous_slice_is_refused_before_the_launch(destination):
    ops = _ops()
    z = torch.randn(1, 4, 4, 8, generator=R.gen(3))
    with pytest.raises(ops.VphoError, match='contiguous'):
        ops.nhwc_to_nchw(z.cuda()[..., ::2])
    assert len(destination) == 1 and destination[0].shape == (1, 4, 4, 4) and _untouched(destination)
    x = z[..., ::2].contiguous()
    got = ops.nhwc_to_nchw(x.cuda())
    assert got is destination[1] and R.bits_equal(got, R.nhwc_to_nchw(x))
