"""Feature-path glue kernels (csrc/misc.hip) one by one against the float64 references of tests/_leaf_fp64.py, on the float32 inputs the
kernel saw, at the shapes where such kernels go wrong: vector / scalar path switches, lane-strided tails, destinations inside wider buffers.

Data movement and single-rounding kernels must match BIT FOR BIT (the build uses -ffp-contract=off).  Arithmetic kernels are held to
R.bound: 4 x the error of torch's own float32 CPU evaluation of the same formula against float64, floor 4 ulp of the largest output
(derivation in tests/_leaf_fp64.py); where the arithmetic gives a bound directly it is derived in the test's docstring."""
import pytest
import torch

from tests import _leaf_fp64 as R

pytestmark = pytest.mark.gpu
SENT = R.SENT


def _ops():
    from vpho_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------ bit-exact group
@pytest.mark.parametrize('N,C,H,W,ld', [(2, 3, 9, 11, 4), (1, 21, 7, 5, 21), (3, 21, 5, 5, 24), (1, 1, 1, 1, 1), (2, 5, 16, 16, 8)])
def test_layout_kernels_move_every_element_and_zero_the_padding(N, C, H, W, ld):
    ops = _ops()
    x = torch.randn(N, C, H, W, generator=R.gen(C * 100 + H))
    y = ops.nchw_to_nhwc(x.cuda(), ld)
    assert R.bits_equal(y, R.nchw_to_nhwc(x, ld))
    assert bool((y[..., C:] == 0).all())
    assert R.bits_equal(ops.nchw_to_nhwc(x.cuda()), R.nchw_to_nhwc(x))
    back = ops.nhwc_to_nchw(y, C)                                     # channels < ld
    assert R.bits_equal(back, x)                                      # the round trip returns the input
    z = torch.randn(N, H, W, ld, generator=R.gen(7))
    assert R.bits_equal(ops.nhwc_to_nchw(z.cuda()), R.nhwc_to_nchw(z))
    assert R.bits_equal(ops.nhwc_to_nchw(z.cuda(), C), R.nhwc_to_nchw(z, C))


@pytest.mark.parametrize('k,stride,pad', [(3, 2, 1), (2, 2, 0)])
@pytest.mark.parametrize('N,H,W,C', [(2, 9, 11, 5), (1, 16, 16, 64), (3, 7, 8, 3)])
def test_maxpool_equals_torch_and_padding_never_wins(k, stride, pad, N, H, W, C):
    ops = _ops()
    x = torch.randn(N, H, W, C, generator=R.gen(H * W + C))
    assert R.bits_equal(ops.maxpool_nhwc(x.cuda(), k, stride, pad), R.maxpool_nhwc(x.double(), k, stride, pad).float())
    neg = -x.abs() - 1.0                                              # all-negative map: a padding value of 0 would win at the border
    got = ops.maxpool_nhwc(neg.cuda(), k, stride, pad)
    assert R.bits_equal(got, R.maxpool_nhwc(neg.double(), k, stride, pad).float()) and bool((got < 0).all())


@pytest.mark.parametrize('bs', [1, 6, 64, 65, 257])
def test_cross_tokens_and_their_adjoint(bs):
    ops = _ops()
    g = R.gen(bs)
    ph, po = torch.randn(bs, 8, 8, 256, generator=g), torch.randn(bs, 8, 8, 256, generator=g)
    ge, pe = torch.randn(bs, 512, generator=g), torch.randn(bs + 3, 512, generator=g)          # pe[b]: one positional row per BATCH index
    got = ops.cross_tokens(ph.cuda(), po.cuda(), ge.cuda(), pe.cuda())
    assert R.bits_equal(got, R.single_rounding(R.cross_tokens, [ph, po, ge, pe]))
    assert not R.bits_equal(got, R.single_rounding(R.cross_tokens, [ph, po, ge, pe[:1].expand(bs + 3, 512)])) or bs == 1
    d = torch.randn(bs, 65, 512, generator=g)
    dph, dpo, dge = ops.cross_tokens_bwd(d.cuda())
    rh, ro, rg = R.cross_tokens_bwd(d)
    assert R.bits_equal(dph, rh) and R.bits_equal(dpo, ro) and R.bits_equal(dge, rg)
    dph, dpo, dge = ops.cross_tokens_bwd(d.cuda(), want_hand=False)   # a detached stream: nothing allocated, the others unchanged
    assert dph is None and R.bits_equal(dpo, ro) and R.bits_equal(dge, rg)
    dph, dpo, dge = ops.cross_tokens_bwd(d.cuda(), want_obj=False)
    assert dpo is None and R.bits_equal(dph, rh)


@pytest.mark.parametrize('n_img,rpi,ldo', [(3, 4, 58), (2, 4 * 5, 58), (5, 1, 64), (1, 7, 61)])
def test_append_betas_writes_columns_48_to_57_only(n_img, rpi, ldo):
    ops = _ops()
    betas = torch.randn(n_img, 10, generator=R.gen(rpi))
    out = torch.full((n_img * rpi, ldo), SENT)
    got = ops.append_betas(betas.cuda(), out.cuda(), rpi)
    assert R.bits_equal(got, R.append_betas(betas, out, rpi))
    assert bool((got[:, :48] == SENT).all()) and bool((got[:, 58:] == SENT).all())
    got3 = ops.append_betas(betas.cuda(), out.view(n_img, rpi, ldo).cuda(), rpi)               # the engine's (bs, S, 58) shape
    assert R.bits_equal(got3.view(-1, ldo), got)


# ------------------------------------------------------------------------------------------------ arithmetic group
RESIZE = [  # N, H, W, C, ldx, OH, OW
    (2, 5, 7, 8, 8, 13, 9), (1, 16, 16, 4, 4, 8, 8), (2, 5, 7, 6, 6, 13, 9), (1, 8, 8, 12, 16, 16, 16), (2, 6, 4, 3, 4, 12, 8),
    (1, 9, 11, 5, 5, 4, 6), (1, 4, 4, 256, 256, 8, 8), (1, 1, 1, 4, 4, 3, 3)]


@pytest.mark.parametrize('N,H,W,C,ldx,OH,OW', RESIZE)
def test_resize_bilinear_against_interpolate(N, H, W, C, ldx, OH, OW):
    """vector path (C, ldx, ldy, c_off all multiples of 4 on 16-byte bases) and scalar path, up- and down-scales, integer and not"""
    ops = _ops()
    x = torch.randn(N, H, W, ldx, generator=R.gen(H * 31 + C))
    ref, tol = R.ruled(R.resize_bilinear_nhwc, [x], OH, OW, C)
    R.check(f'resize_bilinear {H}x{W}->{OH}x{OW} C{C}/ld{ldx}', ops.resize_bilinear_nhwc(x.cuda(), OH, OW, channels=C), ref, tol)
    # a misaligned base pointer must take the scalar path and give the same values
    R.check(f'resize_bilinear misaligned x C{C}', ops.resize_bilinear_nhwc(R.offset_view(x), OH, OW, channels=C), ref, tol)
    out = R.offset_view(torch.zeros(N, OH, OW, C))
    ops.resize_bilinear_nhwc(x.cuda(), OH, OW, out=out, channels=C)
    R.check(f'resize_bilinear misaligned y C{C}', out, ref, tol)


@pytest.mark.parametrize('C,ldy,c_off', [(8, 24, 8), (8, 24, 4), (6, 17, 5), (4, 12, 8), (4, 13, 8)])
@pytest.mark.parametrize('accumulate', [False, True])
def test_resize_bilinear_into_a_wider_buffer(C, ldy, c_off, accumulate):
    ops = _ops()
    N, H, W, OH, OW = 2, 5, 7, 13, 9
    g = R.gen(C * ldy + c_off)
    x, base = torch.randn(N, H, W, C, generator=g), torch.randn(N, OH, OW, ldy, generator=g)
    f = lambda x_, b_: (b_[..., c_off:c_off + C] if accumulate else 0) + R.resize_bilinear_nhwc(x_, OH, OW)
    ref, tol = R.ruled(f, [x, base])
    out = base.cuda()
    ops.resize_bilinear_nhwc(x.cuda(), OH, OW, out=out, c_off=c_off, accumulate=accumulate)
    R.check(f'resize_bilinear c_off {c_off}/{ldy} acc={accumulate}', out[..., c_off:c_off + C], ref, tol)
    keep = torch.ones(ldy, dtype=torch.bool)
    keep[c_off:c_off + C] = False
    assert R.bits_equal(out[..., keep.cuda()], base[..., keep])       # the other channels keep their values


def test_resize_bilinear_pixel_list_touches_listed_pixels_only():
    ops = _ops()
    N, H, W, C, OH, OW = 2, 8, 8, 8, 16, 16
    x = torch.randn(N, H, W, C, generator=R.gen(3))
    boxes = torch.tensor([[8.0, 12.0, 30.0, 40.0], [20.0, 4.0, 60.0, 24.0]])
    win = ops.roi_windows(boxes.cuda(), None, N, OH, OW, 0.25)
    n = int(win.count.item())
    listed = torch.zeros(N * OH * OW, dtype=torch.bool)
    listed[win.row_map[:n].long().cpu()] = True
    listed = listed.view(N, OH, OW)
    assert 0 < n < N * OH * OW
    ref, tol = R.ruled(R.resize_bilinear_nhwc, [x], OH, OW)
    for acc in (False, True):
        out = torch.full((N, OH, OW, C), SENT, device='cuda')
        ops.resize_bilinear_nhwc(x.cuda(), OH, OW, out=out, accumulate=acc, rows=win)
        o = out.cpu()
        assert bool((o[~listed] == SENT).all())
        want = ref[listed] + (SENT if acc else 0.0)
        R.check(f'resize_bilinear rows acc={acc}', o[listed], want, tol + (4 * R.ULP * SENT if acc else 0.0))


@pytest.mark.parametrize('S,C', [(64, 21), (32, 1)])
@pytest.mark.parametrize('kind', ['equal', 'larger', 'smaller'])
def test_align_heatmap_against_gather_and_grid_sample(S, C, kind):
    """quirk Q2: the first output index walks x.  The rectangle's aspect differs from the box's and the map is random, so the exchanged
    reading (i <-> j) is far outside the bound -- asserted below on the reference itself."""
    ops = _ops()
    g = R.gen(S + C)
    N = 4
    hm = torch.rand(N, S, S, C, generator=g)
    bbox, rect = R.boxes(N, g, kind)
    flip = torch.tensor([0, 1, 1, 0], dtype=torch.uint8)              # flipped and unflipped images in one batch
    ref, tol = R.ruled(R.align_heatmap_gather, [hm, bbox, rect], flip)
    ref2 = R.align_heatmap_grid_sample(hm.double(), bbox.double(), rect.double(), flip)
    assert float((ref - ref2).abs().max()) < 1e-12
    got = ops.align_heatmap_nhwc(hm.cuda(), bbox.cuda(), rect.cuda(), flip.cuda())
    R.check(f'align_heatmap S{S} C{C} {kind}', got, ref, tol)
    R.check(f'align_heatmap S{S} C{C} {kind} no flip', ops.align_heatmap_nhwc(hm.cuda(), bbox.cuda(), rect.cuda()),
            R.align_heatmap_gather(hm.double(), bbox.double(), rect.double()), tol)
    if kind == 'larger':
        assert bool((got[:, 0] == 0).all()) and bool((got[:, :, 0] == 0).all()) and bool((got[:, -1] == 0).all())    # outside the map
    swapped = R.align_heatmap_gather(hm.double().transpose(1, 2), bbox.double(), rect.double(), flip)
    assert float((swapped - ref).abs().max()) > 1000 * tol


@pytest.mark.parametrize('N', [1, 64, 257])
def test_nerf_embed(N):
    """the phase g * 2^k is exact in float32 (a power of two), so only sinf / cosf round: the rule's floor (4 ulp of 1, or of the largest
    |g| in the identity block) holds with the <= 2 ulp device functions; column 63 is the zero pad"""
    ops = _ops()
    gen = R.gen(N)
    g = torch.randn(N, 3, generator=gen)
    g = g / g.norm(dim=-1, keepdim=True)
    g[::5, 1] = 10.3 * torch.sign(g[::5, 1])                          # a few components of magnitude ~10 (phases up to ~5000 rad)
    flip = (torch.rand(N, generator=gen) < 0.5).to(torch.uint8)
    for fl in (None, flip):
        ref, tol = R.ruled(R.nerf_embed, [g], fl)
        got = ops.nerf_embed(g.cuda(), None if fl is None else fl.cuda())
        R.check(f'nerf_embed N{N} flip={fl is not None} trig', got[:, 3:63], ref[:, 3:63], min(tol, 4 * R.ULP))
        assert R.bits_equal(got[:, :3], ref[:, :3].float()) and bool((got[:, 63] == 0).all())


@pytest.mark.parametrize('rows', [1, 3, 4, 5, 65 * 64])
@pytest.mark.parametrize('E', [512, 64, 100])
def test_add_layernorm(rows, E):
    ops = _ops()
    g = R.gen(rows + E)
    x, r = torch.randn(rows, E, generator=g), torch.randn(rows, E, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(E, generator=g), 0.1 * torch.randn(E, generator=g)
    ref, tol = R.ruled(R.add_layernorm, [x, r, gamma, beta])
    R.check(f'add_layernorm {rows}x{E}', ops.add_layernorm(x.cuda(), r.cuda(), gamma.cuda(), beta.cuda()), ref, tol)
    # rows whose mean is far above their spread
    x2 = 100 + 0.01 * torch.randn(rows, E, generator=g)
    r2 = 0.001 * torch.randn(rows, E, generator=g)
    ref, tol = R.ruled(R.add_layernorm, [x2, r2, gamma, beta])
    R.check(f'add_layernorm {rows}x{E} mean>>spread', ops.add_layernorm(x2.cuda(), r2.cuda(), gamma.cuda(), beta.cuda()), ref, tol)


@pytest.mark.parametrize('bs', [1, 6, 65])
def test_force_local_engine_addressing_and_contiguous(bs):
    """rows picked out of (bs, 65, .) token-shaped MLP outputs (group 32, stride 65, scale from tokens 0..31, logits from 32..63), the
    contiguous form, a negative scale (|.| is taken), logits of +-80 (the first soft-max saturates) and the double soft-max"""
    ops = _ops()
    g = R.gen(bs)
    scale, logits = torch.randn(bs * 65, 1, generator=g), torch.randn(bs * 65, 8, generator=g) * 3
    scale[::3] = -scale[::3].abs()
    logits[32::7] = torch.tensor([80.0, -80.0, 0.0, 1.0, -1.0, 80.0, 3.0, -80.0])
    anchor = torch.randn(8, 3, generator=g)
    ref, tol = R.ruled(R.force_local, [scale, logits, anchor], bs * 32, 32, 65, 0, 32)
    got = ops.force_local(scale.cuda(), logits.cuda(), anchor.cuda(), bs * 32, 32, 65, 0, 32)
    R.check(f'force_local engine bs{bs}', got, ref, tol)
    single = R.force_local(scale.double(), logits.double(), anchor.double(), bs * 32, 32, 65, 0, 32, double_softmax=False)
    assert float((single - ref).abs().max()) > 1000 * tol             # one soft-max only would be far outside the bound
    pick = lambda t, off: t.view(bs, 65, -1)[:, off:off + 32].reshape(bs * 32, -1).contiguous()
    sc, lg = pick(scale, 0), pick(logits, 32)
    R.check(f'force_local contiguous bs{bs}', ops.force_local(sc.cuda(), lg.cuda(), anchor.cuda(), bs * 32), ref, tol)
    assert R.bits_equal(ops.force_local(sc.cuda(), lg.cuda(), anchor.cuda(), bs * 32), got)
    wide = torch.randn(bs * 32, 12, generator=g)                      # a leading dimension above 8
    ref, tol = R.ruled(R.force_local, [sc, wide, anchor], bs * 32, friction=0.5)
    R.check(f'force_local ld12 bs{bs}', ops.force_local(sc.cuda(), wide.cuda(), anchor.cuda(), bs * 32, friction=0.5), ref, tol)


# ------------------------------------------------------------------------------------------------ argument guards
def test_argument_guards_raise_and_launch_nothing():
    """every documented guard answers VphoError before anything is launched: the destination keeps its sentinel.  Arguments only -- the
    buffers passed are valid for the sizes the call names, or the size named is what the guard rejects."""
    ops = _ops()
    dev = 'cuda'
    sent = lambda *s: torch.full(s, SENT, device=dev)
    out = sent(4, 57)
    with pytest.raises(ops.VphoError):
        ops.append_betas(torch.zeros(1, 10, device=dev), out, 4)      # ldo < 58
    x = torch.zeros(1, 4, 4, 4, device=dev)
    dst = sent(1, 8, 8, 6)
    with pytest.raises(ops.VphoError):
        ops.resize_bilinear_nhwc(x, 8, 8, out=dst, c_off=4)           # ld < c_off + cols
    with pytest.raises(ops.VphoError):
        ops.sum_repeats(torch.zeros(6, 10, device=dev), 8, 3, 2, 4)   # ld < c_off + cols
    tok = sent(1, 65, 512)
    z = torch.zeros(1, 8, 8, 256, device=dev)
    with pytest.raises(ops.VphoError):                               # bs > 5000: by argument, the buffers are never touched
        ops._call('vpho_cross_tokens_f32', z, z, torch.zeros(1, 512, device=dev),
                  torch.zeros(1, 512, device=dev), 5001, tok)
    hm = sent(2, 1, 1, 3)
    box = torch.tensor([[0.0, 0.0, 10.0, 10.0]] * 2, device=dev)
    with pytest.raises(ops.VphoError):
        ops.align_heatmap_nhwc(hm, box, box)                          # size <= 1
    p, gr, m, v = sent(8), torch.ones(8, device=dev), torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    with pytest.raises(ops.VphoError):
        ops.adamw_(p, gr, m, v, 0)                                    # step < 1
    lst = ops.AdamWList([(p, gr, m, v)])
    with pytest.raises(ops.VphoError):
        lst.step(0)
    torch.cuda.synchronize()
    for t in (out, dst, tok, p):
        assert bool((t == SENT).all())
    assert bool((m == 0).all()) and bool((v == 0).all())
