"""Tensor-level wrappers of the C ABI in ``include/vpho_hip.h`` (``vpho_amd/libvpho_hip.so``).

Thin by design: tensors in, plain values to ``abi.call`` out.  Every C type -- struct mirrors, argument and return types -- comes from the
header through ``vpho_amd/abi.py``; no call site here wraps an argument.  There is NO fallback: importing this module without the built
extension raises, and every op checks that its tensors live on a GPU.
"""
import ctypes as C                      # host-side values only: byref, host arrays, struct construction
import os

import torch

from . import abi
from .abi import ABI_VERSION, LIB_PATH, VphoError, lib  # noqa: F401

_call = abi.call                        # a module-level name: tests wrap it to take the census of a step's launches


def _f32p(t):
    """descriptor fields and table records: the checked address of an fp32 tensor"""
    return abi.addr(t, torch.float32)


# ----------------------------------------------------------------------------------------------- conv / linear
ConvDesc = abi.struct('vpho_conv_desc')


FUSE_BN = os.environ.get('VPHO_TRAIN_FUSE_BN', '1') != '0'     # A/B aid: 0 = every train-mode BatchNorm runs its own reduction pass


BN_STAT_PLANES = 6                      # planes of a partial row (include/vpho_hip.h, vpho_conv_desc.stats)


class BnFuse:
    """Carrier of the reductions of a train-mode BatchNorm taken in the epilogue of the convolution next to it (vpho_conv_desc.stats).
    Forward: ``f = BnFuse(); c = conv2d_nhwc(x, w, bn=f); a, saved = bn_train_forward(c, ..., partials=f)`` -- the convolution leaves the
    per-tile sums of its output in ``f.stats`` (``f.rows`` partial rows; 0 = the kernel of that shape has no such epilogue and the
    BatchNorm runs its own pass).  Backward: ``f = BnFuse(c, saved, gamma, beta); da = conv2d_dgrad(dy, w, ..., gate=(a, slope), bn=f)``
    -- the input-gradient convolution recomputes the activation's sign from the BatchNorm input ``c`` instead of reading the stored
    activation and leaves sum da | sum da * xhat -- then ``bn_train_backward(c, da, gamma, saved, partials=f)``."""
    __slots__ = ('stats', 'rows', 'x', 'mean', 'invstd', 'gamma', 'beta', 'stored_gate', 'parts', 'calls', 'failed')

    def __init__(self, x=None, saved=None, gamma=None, beta=None, stored_gate=False, parts=1):
        # stored_gate: keep reading the activation's sign from the stored activation (a residual block's closing activation, whose input is
        # BatchNorm + shortcut) and take only xhat from the BatchNorm input.
        # parts > 1: the map is written by several convolutions, each into its own strided part (the four phases of a transposed convolution
        # / of a stride-2 input gradient, ``out_view``): every launch appends its partial rows; the sums count only when all parts came
        self.stats, self.rows, self.x, self.gamma, self.beta, self.stored_gate = None, 0, x, gamma, beta, stored_gate
        self.mean, self.invstd = saved if saved is not None else (None, None)
        self.parts, self.calls, self.failed = parts, 0, False

    def live(self):
        return self.stats is not None and self.rows > 0 and not self.failed and self.calls == self.parts


# Opt-in split-bf16 convolutions (VPHO_CONV_MFMA=bf16x6|bf16x9, inference plan only; default: fp32 MFMA).  The three bf16 planes of
# a packed weight matrix are made on first use and kept on the tensor object.
import threading
_conv_split = threading.local()


class conv_split:
    """context: convolutions launched inside use split-bf16 products (terms = 6 or 9) where the kernel takes the shape"""
    def __init__(self, terms):
        self.terms = terms

    def __enter__(self):
        self.prev = getattr(_conv_split, 'terms', 0)
        _conv_split.terms = self.terms

    def __exit__(self, *exc):
        _conv_split.terms = self.prev


def bf16_planes(w):
    """(3, *w.shape) bf16 with planes[0] + planes[1] + planes[2] == w exactly (each piece the bf16 rounding of what is left)"""
    h = w.to(torch.bfloat16)
    m = (w - h.float()).to(torch.bfloat16)
    l = (w - h.float() - m.float()).to(torch.bfloat16)
    return torch.stack([h, m, l], 0).contiguous()


def _planes_of(w):
    """the planes live ON the weight tensor object (an address-keyed cache would hand a new tensor at a recycled address the old
    tensor's planes); an in-place update of the weights (``_version``) re-splits them"""
    c = getattr(w, '_vpho_planes', None)
    if c is None or c[0] != w._version:
        c = (w._version, bf16_planes(w))
        w._vpho_planes = c
    return c[1]


def conv2d_nhwc(x, w, bias=None, *, kh=1, kw=1, stride=1, pad=0, pad_y=None, pad_x=None, out=None, out_hw=None,
                out_view=None, res=None, in_scale=None, in_shift=None, in_slope=1.0, out_slope=1.0, cin=None, split=None, gate=None,
                rows=None, rows_scatter=False, res_up=None, x2=None, stride2=1, groups=1, x_shared=False, x2_shared=False, bn=None):
    """x: (N,H,W,x_ld) fp32 NHWC, w: (Cout, kh*kw*Cin) packed.  Returns (N,OH,OW,Cout) (or writes ``out``).
    ``groups`` = G > 1: G convolutions of one shape in ONE launch (the twin hand / object branches, vpho_conv_desc.groups): w (G,Cout,K),
    bias (G,Cout), in_scale / in_shift (G,Cin); x, res, x2, res_up and the result hold the groups' images one after the other
    ((G*N,...): group g = images [g*N, (g+1)*N)); ``x_shared`` / ``x2_shared``: that input is ONE (N,...) tensor read by every group.
    ``res_up`` = a coarser (N,h,w,Cout) map added after bilinear up-sampling to the output grid (the FPN's top-down add fused into the
    lateral convolution, backbone_FPN_HFL.py:66-68; bit-identical to ``resize_bilinear_nhwc(..., accumulate=True)`` after the convolution).
    ``x2`` = a second (N,H2,W2,C2) input of a 1x1 convolution, read at stride ``stride2`` and concatenated behind x along the channels
    (w: (Cout, Cin + C2)): the projection shortcut of a bottleneck merged into conv3 (vpho_conv_desc.x2).

    ``out_view`` = (tensor, y_sn, y_sy, y_sx, element_offset) writes into a strided destination (concat buffers,
    transposed-convolution phases).  ``res`` is a contiguous (N,OH,OW,Cout) tensor.  ``gate`` = (tensor shaped like the
    destination, slope): y = gate > 0 ? y : slope * y (LeakyReLU backward fused into an input-gradient convolution).
    ``rows`` = a ``RoiWindows``: only the listed output pixels are computed and the result is the COMPACT (N*OH*OW, Cout)
    matrix whose first ``rows.count`` rows are live (``roi_align_nhwc(..., win=rows)`` reads it); with ``rows_scatter`` the listed
    pixels are written at their own positions of the ordinary (N,OH,OW,Cout) output and the other pixels are left untouched.
    ``bn`` = a ``BnFuse``: the reductions of the train-mode BatchNorm next to this convolution in its epilogue (see BnFuse; with
    ``bn.x`` the gate is recomputed from the BatchNorm input and ``gate`` -- which the caller still passes -- is used only where the
    fused epilogue does not apply)."""
    N, H, W, x_ld = x.shape
    G = groups
    if G > 1:
        assert w.dim() == 3 and w.shape[0] == G and w.is_contiguous() and (bias is None or (bias.shape == (G, w.shape[1]) and bias.is_contiguous()))
        assert rows is None and split is None and gate is None and x.is_contiguous()
        if not x_shared:
            assert N % G == 0, (N, G)
            N //= G
    cin = x_ld if cin is None else cin
    cout = w.shape[-2]
    assert split is not None or w.shape[-1] == kh * kw * cin + (0 if x2 is None else x2.shape[-1]), (w.shape, kh, kw, cin)
    py = pad if pad_y is None else pad_y
    px = pad if pad_x is None else pad_x
    if out_hw is None:
        OH, OW = (H + 2 * py - kh) // stride + 1, (W + 2 * px - kw) // stride + 1
    else:
        OH, OW = out_hw
    d = ConvDesc()
    d.x, d.w, d.bias = _f32p(x), _f32p(w), _f32p(bias)
    d.in_scale, d.in_shift, d.res = _f32p(in_scale), _f32p(in_shift), _f32p(res)
    if rows is not None:
        assert out_view is None and res is None and gate is None and rows.shape == (N, OH, OW) and (res_up is None or rows_scatter)
        if out is None:
            out = torch.empty((N, OH, OW, cout) if rows_scatter else (N * OH * OW, cout), device=x.device, dtype=torch.float32)
        _f32p(out)
        ld = out.shape[-1]
        d.y, d.y_sx, d.y_sy, d.y_sn = out.data_ptr(), ld, (ld * OW if rows_scatter else 0), (ld * OW * OH if rows_scatter else 0)
        d.rows_scatter = 1 if rows_scatter else 0
        d.row_map, d.row_count = rows.row_map.data_ptr(), rows.count.data_ptr()
        d.rows_hint = int(rows.count.item()) if _prof_on else 0      # the instrumented pass may synchronise; the product path never does
        ret = out
    elif out_view is not None:
        yt, d.y_sn, d.y_sy, d.y_sx, off = out_view
        _f32p(yt)
        d.y = yt.data_ptr() + 4 * off
        ret = yt
        if gate is not None:
            assert gate[0].shape == yt.shape and gate[0].is_contiguous() and yt.is_contiguous()
            d.gate, d.gate_slope = _f32p(gate[0]) + 4 * off, gate[1]
    else:
        if out is None:
            out = torch.empty((G * N, OH, OW, cout), device=x.device, dtype=torch.float32)
        _f32p(out)
        assert out.shape[0] == G * N
        ld = out.shape[-1]
        d.y, d.y_sx, d.y_sy, d.y_sn = out.data_ptr(), ld, ld * OW, ld * OW * OH
        ret = out
        if gate is not None:
            assert gate[0].shape == out.shape
            d.gate, d.gate_slope = _f32p(gate[0]), gate[1]
    if res is not None:
        assert res.shape == (G * N, OH, OW, cout)
        d.r_sx, d.r_sy, d.r_sn = cout, cout * OW, cout * OW * OH
    if x2 is not None:
        assert kh == kw == 1 and rows is None and split is None and in_scale is None and x2.shape[0] == (N if (G == 1 or x2_shared) else G * N) and x2.is_contiguous()
        d.x2, d.Cin2, d.x2_ld, d.stride2, d.H2, d.W2 = _f32p(x2), x2.shape[3], x2.shape[3], stride2, x2.shape[1], x2.shape[2]
    if res_up is not None:
        assert res is None and res_up.shape[0] == G * N and res_up.shape[3] == cout and res_up.is_contiguous()
        d.res_up, d.ru_H, d.ru_W, d.ru_ld = _f32p(res_up), res_up.shape[1], res_up.shape[2], res_up.shape[3]
    if G > 1:
        assert in_scale is None or (in_scale.shape == (G, cin) and in_shift.shape == (G, cin) and in_scale.is_contiguous() and in_shift.is_contiguous())
        d.groups = G
        d.x_group = 0 if x_shared else N * H * W * x_ld
        # a strided destination (out_view: transposed-convolution phases) holds the groups' images one after the other as well
        d.w_group, d.bias_group, d.y_group = w.shape[1] * w.shape[2], cout, (ret.numel() // G if out_view is not None else N * OH * OW * ret.shape[-1])
        d.res_group = N * OH * OW * cout
        d.x2_group = 0 if (x2 is None or x2_shared) else N * x2.shape[1] * x2.shape[2] * x2.shape[3]
        d.pre_group = cin
        d.ru_group = 0 if res_up is None else N * res_up.shape[1] * res_up.shape[2] * res_up.shape[3]
    d.N, d.H, d.W, d.Cin, d.x_ld = N, H, W, cin, x_ld
    d.Cout, d.KH, d.KW, d.stride, d.pad_y, d.pad_x, d.OH, d.OW = cout, kh, kw, stride, py, px, OH, OW
    d.in_slope, d.out_slope = in_slope, out_slope
    if split is not None:                                   # (splits, w_ld, x_split, w_split, y_split): see vpho_conv_desc
        d.splits, d.w_ld, d.x_split, d.w_split, d.y_split = split
    terms = getattr(_conv_split, 'terms', 0)
    if terms and G == 1 and split is None and in_scale is None and gate is None and res_up is None and x2 is None and cin % 16 == 0 and w.is_contiguous() and w.shape[1] == kh * kw * cin:
        planes = _planes_of(w)                              # kept alive by the cache
        d.w_planes, d.plane_terms = planes.data_ptr(), terms
    rows_out = None
    if bn is not None and FUSE_BN and G == 1 and split is None and rows is None and in_scale is None and (out_view is None or bn.parts > 1) and not d.w_planes and cout % 4 == 0:
        cap = (N * OH * OW + 63) // 64                          # the smallest M-tile is 64 rows
        if bn.stats is None:
            bn.stats = torch.empty((cap * bn.parts, BN_STAT_PLANES, cout), device=x.device, dtype=torch.float32)
        base = bn.rows                                          # parts > 1: this launch appends behind the rows of the earlier parts
        assert base + cap <= bn.stats.shape[0] and bn.stats.shape[2] == cout
        rows_out = C.c_int(0)
        d.stats, d.stats_cap, d.stats_rows = bn.stats.data_ptr() + base * BN_STAT_PLANES * cout * 4, cap, C.addressof(rows_out)
        if bn.x is not None:
            assert gate is not None and bn.x.shape == ret.shape and bn.x.is_contiguous() and ret.is_contiguous()
            bx = _f32p(bn.x) + (4 * out_view[4] if out_view is not None else 0)      # laid out like y, like the gate
            if bn.stored_gate:
                d.bn_x, d.bn_mean, d.bn_invstd = bx, _f32p(bn.mean), _f32p(bn.invstd)
            else:                                               # gate recomputed; the stored gate stays as the kernel's fall-back
                d.bn_x = bx
                d.bn_mean, d.bn_invstd, d.bn_gamma, d.bn_beta = (_f32p(t) for t in (bn.mean, bn.invstd, bn.gamma, bn.beta))
    elif bn is not None:
        bn.failed = True
    _call('vpho_conv2d_nhwc_f32', C.byref(d))
    if rows_out is not None:
        bn.calls += 1
        if rows_out.value == 0:
            bn.failed = True
        bn.rows += rows_out.value
    return ret


def conv3x3(x, w, bias=None, out_slope=1.0, winograd=True, rows=None, groups=1, x_shared=False):
    """3x3 / stride 1 / pad 1 convolution + bias + LeakyReLU of the inference plan: the Winograd F(2x2,3x3) kernel where its shape
    conditions hold (even H and W, Cin % 16 == 0, Cout % 64 == 0), else the direct implicit GEMM.  The transformed weights live on the
    weight tensor object and follow its version.  ``rows`` = a ``RoiWindows``: only the window pixels, as the compact (N*H*W, Cout)
    matrix (see conv2d_nhwc).  ``groups``: see conv2d_nhwc (w (G,Cout,9*Cin))."""
    N, H, W, x_ld = x.shape
    cout, k9 = w.shape[-2:]
    cin = k9 // 9
    if not winograd or H % 2 or W % 2 or cin % 16 or cout % 64 or x_ld != cin:
        return conv2d_nhwc(x, w, bias, kh=3, kw=3, pad=1, out_slope=out_slope, rows=rows, groups=groups, x_shared=x_shared)
    c = getattr(w, '_vpho_wino', None)
    if c is None or c[0] != w._version:
        from .model.pack import winograd_weights
        c = (w._version, winograd_weights(w) if groups == 1 else torch.stack([winograd_weights(w[g]) for g in range(groups)]).contiguous())
        w._vpho_wino = c
    return conv3x3_winograd(x, c[1], bias, out_slope, rows=rows, groups=groups, x_shared=x_shared)


def conv3x3_winograd(x, u, bias=None, out_slope=1.0, out=None, rows=None, groups=1, x_shared=False):
    """3x3 / stride 1 / pad 1 convolution in Winograd F(2x2,3x3) form; u = pack.winograd_weights(packed weights) (Cin/8, 16, Cout, 8);
    groups = G > 1: u (G, Cin/8, 16, Cout, 8), bias (G, Cout), x (G*N,H,W,Cin) or one shared (N,H,W,Cin) -> (G*N,H,W,Cout)"""
    N, H, W, x_ld = x.shape
    cout, cin = u.shape[-2], u.shape[-4] * 8
    assert u.shape[-3] == 16 and u.shape[-1] == 8
    if groups > 1:
        assert rows is None and u.dim() == 5 and u.shape[0] == groups and u.is_contiguous() and x.is_contiguous() and (bias is None or bias.shape == (groups, cout))
        if not x_shared:
            assert N % groups == 0
            N //= groups
        if out is None:
            out = torch.empty((groups * N, H, W, cout), device=x.device, dtype=torch.float32)
        _call('vpho_conv3x3_winograd_grouped_nhwc_f32', x, 0 if x_shared else N * H * W * x_ld, u, bias, groups, N, H, W, cin, x_ld, cout, out_slope,
              out, out.shape[-1])
        return out
    if rows is not None:
        assert rows.shape == (N, H, W)
        if out is None:
            out = torch.empty((N * H * W, cout), device=x.device, dtype=torch.float32)
        _call('vpho_conv3x3_winograd_rows_nhwc_f32', x, u, bias, N, H, W, cin, x_ld, cout, out_slope, rows.wins, rows.tiles(),
              int(rows.tiles()[N].item()) if _prof_on else 0, out, out.shape[-1])
        return out
    if out is None:
        out = torch.empty((N, H, W, cout), device=x.device, dtype=torch.float32)
    _call('vpho_conv3x3_winograd_nhwc_f32', x, u, bias, N, H, W, cin, x_ld, cout, out_slope, out, out.shape[-1])
    return out


def winograd_weights_device(w, for_input_gradient=False):
    """u of pack.winograd_weights made on the DEVICE (training: the weights change every step, a host transform would synchronise),
    for the forward convolution or for its input-gradient convolution; kept on the weight tensor object, follows its version"""
    key = '_vpho_wino_dev_t' if for_input_gradient else '_vpho_wino_dev'
    c = getattr(w, key, None)
    if c is None or c[0] != w._version:
        cout, k9 = w.shape
        cin = k9 // 9
        o, i = (cin, cout) if for_input_gradient else (cout, cin)
        u = c[1] if c is not None else torch.empty((i // 8, 16, o, 8), device=w.device, dtype=torch.float32)
        _call('vpho_winograd_weights_f32', w, cout, cin, 1 if for_input_gradient else 0, u)
        c = (w._version, u)
        setattr(w, key, c)
        if _WINO_BATCH is not None:
            _WINO_BATCH.add(w, key, 1 if for_input_gradient else 0, u)
    return c[1]


class WinogradWeightBatch:
    """Every transform requested inside ``with batch:`` is remembered; ``refresh()`` (after the optimiser step) redoes ALL of them with one
    launch (vpho_winograd_weights_multi_f32) and marks them current, so the step's convolutions find them ready -- instead of one small
    launch in front of each of the step's 81 Winograd convolutions."""

    def __init__(self):
        self.items, self.table, self.blocks = {}, None, 0

    def __enter__(self):
        global _WINO_BATCH
        self._outer, _WINO_BATCH = _WINO_BATCH, self
        return self

    def __exit__(self, *exc):
        global _WINO_BATCH
        _WINO_BATCH = self._outer

    def add(self, w, key, mode, u):
        k = (w.data_ptr(), key)
        if k not in self.items:
            self.items[k] = (w, key, mode, u)              # keeps w alive: its address stays its own
            self.table = None

    def refresh(self):
        if not self.items:
            return
        if self.table is None:
            import numpy as np
            rec = np.zeros(len(self.items), dtype=[('w', '<u8'), ('u', '<u8'), ('cout', '<i4'), ('cin', '<i4'), ('mode', '<i4'), ('blk0', '<i4')])
            blk = 0
            for n, (w, key, mode, u) in enumerate(self.items.values()):
                cout, cin = w.shape[0], w.shape[1] // 9
                _f32p(w), _f32p(u)
                rec[n] = (w.data_ptr(), u.data_ptr(), cout, cin, mode, blk)
                blk += (cout * cin + 255) // 256
            dev = next(iter(self.items.values()))[0].device
            self.table, self.blocks = torch.from_numpy(rec.view(np.uint8).copy()).to(dev), blk
        _call('vpho_winograd_weights_multi_f32', abi.at(self.table, torch.uint8), len(self.items), self.blocks)
        for w, key, mode, u in self.items.values():
            setattr(w, key, (w._version, u))


_WINO_BATCH = None


def winograd_ok(H, W, cin, cout, x_ld):
    return H % 2 == 0 and W % 2 == 0 and cin % 16 == 0 and cout % 64 == 0 and x_ld == cin and not getattr(_conv_split, 'terms', 0)


_TRAIN_WINOGRAD = os.environ.get('VPHO_TRAIN_WINOGRAD', '1') != '0'


def _winograd_bn(x, u, bias, out_slope, cin, cout, bn, gate_slope=1.0):
    """full-map Winograd convolution with the BatchNorm reductions in its epilogue (vpho_conv3x3_winograd_stats_nhwc_f32)"""
    N, H, W, x_ld = x.shape
    out = torch.empty((N, H, W, cout), device=x.device, dtype=torch.float32)
    cap = (N * H * W + 255) // 256
    bn.stats = torch.empty((cap, BN_STAT_PLANES, cout), device=x.device, dtype=torch.float32)
    rows_out = C.c_int(0)
    b_x, b_mean, b_invstd, b_gamma, b_beta = (bn.x, bn.mean, bn.invstd, bn.gamma, bn.beta) if bn.x is not None else (None,) * 5
    if bn.x is not None:
        assert bn.x.shape == out.shape and bn.x.is_contiguous()
    _call('vpho_conv3x3_winograd_stats_nhwc_f32', x, u, bias, N, H, W, cin, x_ld, cout, out_slope, out, cout, bn.stats, cap, C.byref(rows_out), b_x,
          b_mean, b_invstd, b_gamma, b_beta, gate_slope)
    bn.rows, bn.calls = rows_out.value, 1
    return out


def conv3x3_train(x, w, bias=None, out_slope=1.0, rows=None, bn=None):
    """3x3 / stride 1 / pad 1 convolution of the TRAINING path: Winograd F(2x2,3x3) with the weight transform on the device where the
    shape allows, else the direct kernel (VPHO_TRAIN_WINOGRAD=0: always the direct kernel).  ``rows`` (a RoiWindows): the output is
    only ever read inside these windows (RoIAlign), so only their pixels are computed -- in place in the ordinary (N,H,W,Cout) map,
    zeros elsewhere; same values as the full convolution on every window pixel."""
    N, H, W, x_ld = x.shape
    cout, cin = w.shape[0], w.shape[1] // 9
    if not _TRAIN_WINOGRAD or not winograd_ok(H, W, cin, cout, x_ld) or w.shape[1] != 9 * cin:
        return conv2d_nhwc(x, w, bias, kh=3, kw=3, pad=1, out_slope=out_slope, bn=bn)
    u = winograd_weights_device(w)
    if bn is not None and FUSE_BN and rows is None:
        return _winograd_bn(x, u, bias, out_slope, cin, cout, bn)
    if rows is not None:
        assert rows.shape == (N, H, W)
        out = torch.zeros((N, H, W, cout), device=x.device, dtype=torch.float32)
        _call('vpho_conv3x3_winograd_scatter_nhwc_f32', x, u, bias, N, H, W, cin, x_ld, cout, out_slope, rows.wins, rows.tiles(), out, cout)
        return out
    return conv3x3_winograd(x, u, bias, out_slope)


def conv3x3_dgrad_winograd(dy, w, gate=None, rows=None, bn=None):
    """input gradient of a 3x3 / stride 1 / pad 1 convolution with packed weights w (Cout, 9*Cin): dX = conv3x3(dY, flipped / transposed
    w), optionally through the backward of the LeakyReLU that produced the convolution's input (gate = (that input, slope)).
    ``rows`` (a RoiWindows, no gate): dY is zero outside the windows' interior, so dX is computed on the window pixels only and is
    zero elsewhere.  None when the shape is not one the Winograd kernel takes (the caller then uses the direct kernel)."""
    N, H, W, ld = dy.shape
    cout, cin = w.shape[0], w.shape[1] // 9
    if not _TRAIN_WINOGRAD or not winograd_ok(H, W, cout, cin, ld) or w.shape[1] != 9 * cin:
        return None
    u = winograd_weights_device(w, for_input_gradient=True)
    if rows is not None and gate is None:
        assert rows.shape == (N, H, W)
        out = torch.zeros((N, H, W, cin), device=dy.device, dtype=torch.float32)
        _call('vpho_conv3x3_winograd_scatter_nhwc_f32', dy, u, None, N, H, W, cout, ld, cin, 1.0, rows.wins, rows.tiles(), out, cin)
        return out
    if gate is None:
        return conv3x3_winograd(dy, u, None, 1.0)
    g, slope = gate
    if bn is not None and bn.x is not None and FUSE_BN:
        return _winograd_bn(dy, u, None, 1.0, cout, cin, bn, gate_slope=slope)
    assert g.shape == (N, H, W, cin) and g.is_contiguous()
    out = torch.empty((N, H, W, cin), device=dy.device, dtype=torch.float32)
    _call('vpho_conv3x3_winograd_gate_nhwc_f32', dy, u, g, slope, N, H, W, cout, ld, cin, out, cin)
    return out


def linear(x, w, bias=None, out_slope=1.0, out=None, acc64=False):
    """x: (rows, cin) fp32, w: (cout, cin) -> (rows, cout).  Same kernel as conv2d_nhwc (1x1).  ``acc64``: products and sum in double,
    one rounding (vpho_linear_acc64_f32: the regression head, whose rounding noise the 6-D normalisation amplifies into the candidates)"""
    rows, cin = x.shape
    if acc64:
        assert x.is_contiguous() and w.is_contiguous() and w.shape[1] == cin
        y = torch.empty((rows, w.shape[0]), device=x.device, dtype=torch.float32) if out is None else out
        _call('vpho_linear_acc64_f32', x, rows, cin, cin, w, bias, w.shape[0], out_slope, y, y.shape[-1])
        return y
    y = conv2d_nhwc(x.view(rows, 1, 1, cin), w, bias, out_slope=out_slope,
                    out=None if out is None else out.view(rows, 1, 1, w.shape[0]))
    return y.view(rows, w.shape[0])


# ----------------------------------------------------------------------------------------------- score net / sampler
ScoreWeights = abi.struct('vpho_score_weights')
OdeStats = abi.struct('vpho_ode_stats')


class ScoreNet:
    """Packed weights of one BaseDenoiser (keeps the device tensors alive) + scratch."""

    def __init__(self, sd, prefix, device):
        g = lambda k: sd[f'{prefix}.{k}'].detach().to(device=device, dtype=torch.float32)
        w1, b1 = g('head.head.0.weight'), g('head.head.0.bias')          # (n,1408,256), (n,256)
        w2, b2 = g('head.head.2.weight'), g('head.head.2.bias')          # (n,256,3), (n,3)
        n = w1.shape[0]
        self.nheads, self.D = n, 3 * n
        self.Dp = (self.D + 3) // 4 * 4
        NH = n * 256
        pe0 = g('pose_encoder.0.weight')                                 # (256, D)
        t = dict(
            t_W=g('t_encoder.0.W').contiguous(), t_w=g('t_encoder.1.weight').contiguous(), t_b=g('t_encoder.1.bias').contiguous(),
            pe0_w=torch.nn.functional.pad(pe0, (0, self.Dp - self.D)).contiguous(), pe0_b=g('pose_encoder.0.bias').contiguous(),
            pe2_w=g('pose_encoder.2.weight').contiguous(), pe2_b=g('pose_encoder.2.bias').contiguous(),
            w1_t=w1[:, :128, :].permute(1, 0, 2).reshape(128, NH).contiguous(),
            w1_p=w1[:, 128:384, :].permute(0, 2, 1).reshape(NH, 256).contiguous(),
            w1_f=w1[:, 384:, :].permute(0, 2, 1).reshape(NH, 1024).contiguous(),
            b1=b1.reshape(NH).contiguous(),
            w2=torch.nn.functional.pad(w2, (0, 1)).reshape(NH, 4).contiguous(), b2=b2.reshape(n * 3).contiguous())
        self.tensors = t
        self.c = ScoreWeights()
        self.c.D, self.c.Dp, self.c.nheads = self.D, self.Dp, n
        for k, v in t.items():
            setattr(self.c, k, v.data_ptr())
        self.device = device
        self._ws = None
        self.set_split(os.environ.get('VPHO_SCORE_MFMA', 'f32'))

    def set_split(self, mode):
        """'f32' (default: fp32 MFMA) | 'bf16x6' | 'bf16x9': the score head's 256 x 256 layer as split-bf16 products (opt-in)"""
        terms = {'f32': 0, 'bf16x6': 6, 'bf16x9': 9}[mode]
        if terms and 'w1_p_split' not in self.tensors:
            w = self.tensors['w1_p'].view(self.nheads, 256, 256)
            h = w.to(torch.bfloat16)
            m = (w - h.float()).to(torch.bfloat16)
            l = (w - h.float() - m.float()).to(torch.bfloat16)
            assert torch.equal(h.float() + m.float() + l.float(), w)       # three 8-bit pieces hold an fp32 exactly
            self.tensors['w1_p_split'] = torch.stack([h, m, l], 1).contiguous()      # (n, 3, 256, 256)
        self.c.w1_p_split = self.tensors['w1_p_split'].data_ptr() if terms else None
        self.c.split_terms = terms
        self.split_mode = mode

    def workspace(self, bs, S):
        need = abi.query('vpho_score_workspace_bytes', C.byref(self.c), bs, S)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def score(self, feat_img, x, t, S):
        """feat_img (bs,1024), x (bs*S, D), scalar t -> score (bs*S, D)   [denoiser.py:68-82]"""
        bs = feat_img.shape[0]
        ws = self.workspace(bs, S)
        out = torch.empty((bs * S, self.D), device=self.device, dtype=torch.float32)
        _call('vpho_score_eval', C.byref(self.c), feat_img, bs, S, x, float(t), out, ws, ws.numel())
        return out

    def sample(self, feat_img, init_x, S, T0, num_steps, xs_f64, x_f64=True, eps=1e-5, rtol=3e-3, atol=3e-4, log_cap=4096):
        """cond_ode_sampler (score_based_model.py:45-105).  Returns xs (R,steps,D), x (R,D), stats dict."""
        bs = feat_img.shape[0]
        R = bs * S
        assert init_x.shape == (R, self.D)
        ws = self.workspace(bs, S)
        xs = torch.empty((R, num_steps, self.D), device=self.device, dtype=torch.float64 if xs_f64 else torch.float32)
        x = torch.empty((R, self.D), device=self.device, dtype=torch.float64 if x_f64 else torch.float32)
        st = OdeStats()
        log = (C.c_double * (4 * log_cap))()
        _call('vpho_ode_sample', C.byref(self.c), feat_img, bs, S, init_x, float(T0), float(eps), int(num_steps), float(rtol), float(atol), xs,
              1 if xs_f64 else 0, x, 1 if x_f64 else 0, ws, ws.numel(), C.byref(st), log, log_cap)
        n = min(st.n_log, log_cap)
        steps = [(log[4 * i], log[4 * i + 1], log[4 * i + 2], bool(log[4 * i + 3])) for i in range(n)]
        return xs, x, dict(nfev=st.nfev, n_accepted=st.n_accepted, n_rejected=st.n_rejected, nan_count=st.nan_count,
                           steps=steps)


# ----------------------------------------------------------------------------------------------- glue kernels
def _new(shape, like, dtype=torch.float32):
    return torch.empty(shape, device=like.device, dtype=dtype)


def nchw_to_nhwc(x, ld=None):
    N, Cc, H, W = x.shape
    ld = Cc if ld is None else ld
    y = _new((N, H, W, ld), x)
    _call('vpho_nchw_to_nhwc_f32', x, N, Cc, H, W, y, ld)
    return y


def nhwc_to_nchw(x, channels=None):
    N, H, W, ld = x.shape
    Cc = ld if channels is None else channels
    y = _new((N, Cc, H, W), x)
    _call('vpho_nhwc_to_nchw_f32', x, N, H, W, Cc, ld, y)
    return y


def maxpool_nhwc(x, k, stride, pad):
    N, H, W, Cc = x.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = _new((N, OH, OW, Cc), x)
    _call('vpho_maxpool_nhwc_f32', x, N, H, W, Cc, k, stride, pad, y)
    return y


def resize_bilinear_nhwc(x, OH, OW, out=None, c_off=0, accumulate=False, channels=None, rows=None):
    N, H, W, ldx = x.shape
    Cc = ldx if channels is None else channels
    if out is None:
        out = _new((N, OH, OW, Cc), x)
    assert out.shape[:3] == (N, OH, OW)
    if rows is not None:                                     # only the listed output pixels (RoiWindows), in place
        assert rows.shape == (N, OH, OW)
        _call('vpho_resize_bilinear_rows_nhwc_f32', x, N, H, W, Cc, ldx, OH, OW, out, out.shape[-1], c_off, 1 if accumulate else 0, rows.row_map,
              rows.count, int(rows.count.item()) if _prof_on else 0)
        return out
    _call('vpho_resize_bilinear_nhwc_f32', x, N, H, W, Cc, ldx, OH, OW, out, out.shape[-1], c_off, 1 if accumulate else 0)
    return out


class RoiWindows:
    """Per-image pixel windows of a feature map (device data): ``wins`` (N,5) int32 = (first row, y0, x0, w, h), ``row_map``
    the linear pixel index of every window pixel, ``count`` (1,) their number.  See vpho_roi_windows_i32."""
    def __init__(self, wins, row_map, count, shape):
        self.wins, self.row_map, self.count, self.shape = wins, row_map, count, shape
        self._tiles = None

    def tiles(self):
        """(N+1,) int32: first 2 x 2 Winograd tile of every image's window, [N] = their number (vpho_winograd_window_tiles_i32)"""
        if self._tiles is None:
            self._tiles = torch.empty((self.shape[0] + 1,), device=self.wins.device, dtype=torch.int32)
            _call('vpho_winograd_window_tiles_i32', self.wins, self.shape[0], self._tiles)
        return self._tiles

    def to_map(self, rows):
        """Inspection helper (synchronises): the compact matrix scattered back to (N,H,W,C), zeros outside the windows, and the
        (N,H,W) mask of the window pixels."""
        n = int(self.count.item())
        N, H, W = self.shape
        idx = self.row_map[:n].long()
        full = torch.zeros((N * H * W, rows.shape[-1]), device=rows.device, dtype=rows.dtype)
        full[idx] = rows[:n]
        mask = torch.zeros((N * H * W,), device=rows.device, dtype=torch.bool)
        mask[idx] = True
        return full.view(N, H, W, -1), mask.view(N, H, W)


def roi_windows(boxes_a, boxes_b, N, H, W, spatial_scale, dilate=0):
    dev = boxes_a.device
    wins = torch.empty((N, 5), device=dev, dtype=torch.int32)
    row_map = torch.empty((N * H * W,), device=dev, dtype=torch.int32)
    count = torch.empty((1,), device=dev, dtype=torch.int32)
    _call('vpho_roi_windows_i32', boxes_a, boxes_b, N, H, W, spatial_scale, dilate, wins, row_map, count)
    return RoiWindows(wins, row_map, count, (N, H, W))


def roi_align_nhwc(feat, boxes, out_size, spatial_scale, flip_w=None, out=None, c_off=0, win=None):
    if win is not None:                                      # feat = compact (rows, C) matrix of the windows' pixels
        N, H, W = win.shape
        Cc = feat.shape[-1]
        if out is None:
            out = _new((N, out_size, out_size, Cc), feat)
        _call('vpho_roi_align_window_nhwc_f32', feat, win.wins, N, H, W, Cc, boxes, spatial_scale, out_size, flip_w, out, out.shape[-1], c_off,
              int(win.count.item()) if _prof_on else 0)
        return out
    N, H, W, Cc = feat.shape
    if out is None:
        out = _new((N, out_size, out_size, Cc), feat)
    _call('vpho_roi_align_nhwc_f32', feat, N, H, W, Cc, boxes, spatial_scale, out_size, flip_w, out, out.shape[-1], c_off)
    return out


def roi_align_dual_nhwc(feat, boxes, out_size, spatial_scale, win, out2, flip_w2=None, c_off2=0, out=None):
    """one pooling pass over the compact window matrix, two destinations: returns the plain crop (new tensor, or ``out``) and writes the
    same values into ``out2`` at channel offset ``c_off2`` under ``flip_w2`` (vpho_roi_align_window_dual_nhwc_f32)"""
    N, H, W = win.shape
    Cc = feat.shape[-1]
    if out is None:
        out = _new((N, out_size, out_size, Cc), feat)
    assert out.shape == (N, out_size, out_size, Cc) and out.is_contiguous()
    _call('vpho_roi_align_window_dual_nhwc_f32', feat, win.wins, N, H, W, Cc, boxes, spatial_scale, out_size, None, out, Cc, 0, flip_w2, out2,
          out2.shape[-1], c_off2, int(win.count.item()) if _prof_on else 0)
    return out


def align_heatmap_nhwc(hm, bbox, bbox_rect, flip_w=None):
    N, S, _, Cc = hm.shape
    out = torch.empty_like(hm)
    _call('vpho_align_heatmap_nhwc_f32', hm, N, S, Cc, bbox, bbox_rect, flip_w, out)
    return out


def nerf_embed(g, flip_x=None):
    N = g.shape[0]
    out = _new((N, 64), g)
    _call('vpho_nerf_embed_f32', g, N, flip_x, out)
    return out


def cross_tokens(proj_hand, proj_obj, grav_emb, pe):
    bs = proj_hand.shape[0]
    out = _new((bs, 65, 512), proj_hand)
    _call('vpho_cross_tokens_f32', proj_hand, proj_obj, grav_emb, pe, bs, out)
    return out


def mha(qkv, S, B, E, nhead, drop=None):
    """drop: optional (B*nhead, S, S) keep-mask / (1 - p) on the attention probabilities (training)"""
    out = _new((S, B, E), qkv)
    _call('vpho_mha_dropout_f32', qkv, S, B, E, nhead, drop, out)
    return out


def add_layernorm(x, r, gamma, beta, eps=1e-5):
    E = x.shape[-1]
    out = torch.empty_like(x)
    _call('vpho_add_layernorm_f32', x, r, gamma, beta, x.numel() // E, E, eps, out)
    return out


def force_local(scale, logits, anchor, rows, group=1, group_stride=1, off_scale=0, off_logits=0, friction=0.8):
    out = _new((rows, 3), scale)
    _call('vpho_force_local_f32', scale, scale.shape[1], logits, logits.shape[1], anchor, friction, rows, group, group_stride, off_scale, off_logits,
          out)
    return out


def rot6d_to_axis_angle(x, rot_per_row, out=None, ldo=None):
    rows, ldx = x.shape
    if out is None:
        out = _new((rows, 3 * rot_per_row), x)
    _call('vpho_rot6d_to_axis_angle_f32', x, rows, rot_per_row, ldx, out, out.shape[-1] if ldo is None else ldo)
    return out


def append_betas(betas, out, rows_per_image):
    rows = out.numel() // out.shape[-1]
    _call('vpho_append_betas_f32', betas, rows, rows_per_image, out, out.shape[-1])
    return out


# ----------------------------------------------------------------------------------------------- MANO
ManoTables = abi.struct('vpho_mano_tables')


class Mano:
    def __init__(self, mano, device):
        t = lambda a: torch.as_tensor(a, dtype=torch.float32).to(device).contiguous()
        self.tensors = dict(v_template=t(mano['v_template']), shapedirs=t(mano['shapedirs']),
                            posedirs_t=t(mano['posedirs']).reshape(778 * 3, 135).t().contiguous(),
                            J_regressor=t(mano['J_regressor']), weights=t(mano['weights']))
        tips = [745, 317, 444, 556, 673, 728, 353, 442, 576, 694]                   # manopth tips, then the HO3D ones (csrc/mano.hip)
        cols = torch.tensor([3 * v + c for v in tips for c in range(3)], device=device)
        self.tensors['tip_posedirs_t'] = self.tensors['posedirs_t'][:, cols].contiguous()     # (135, 30)
        # the table in the operand order of the matrix-core kernel (include/vpho_hip.h): k = 2 (4 g + sl) + lh, vertex = 32 t + li
        pad = torch.zeros((136, 800, 3), device=device, dtype=torch.float32)
        pad[:135, :778] = self.tensors['posedirs_t'].view(135, 778, 3)
        frag = pad.view(17, 4, 2, 25, 32, 3).permute(3, 0, 2, 4, 1, 5).reshape(25, 17, 2, 32, 3, 4)        # [t][g][lh][li][j][e]
        self.tensors['posedirs_mfma'] = frag.permute(0, 1, 4, 2, 3, 5).contiguous()                            # [t][g][j][lh][li][e]
        self.c = ManoTables()
        for k, v in self.tensors.items():
            setattr(self.c, k, v.data_ptr())

    def shape(self, betas):
        n = betas.shape[0]
        vs, J = _new((n, 778, 3), betas), _new((n, 16, 3), betas)
        _call('vpho_mano_shape_f32', C.byref(self.c), betas, n, vs, J)
        return vs, J

    def train(self, rot6d, shape, gt_vert, gt_joint, gt_rot6d, gt_shape, is_right, weights, want_outputs=False, is_ho3d=None):
        """HeadMano tail in training mode (vpho_mano_train_f32): -> losses dict (0-d fp64 tensors, weighted), d_rot6d (bs,96),
        d_shape (bs,10)[, verts, joints]; weights = (vert, joint, mano_pose, mano_shape)"""
        bs = rot6d.shape[0]
        d6, ds = torch.empty_like(rot6d), torch.empty_like(shape)
        parts = _new((bs, 4), rot6d, torch.float64)
        verts = _new((bs, 778, 3), rot6d) if want_outputs else None
        joints = _new((bs, 21, 3), rot6d) if want_outputs else None
        _call('vpho_mano_train_f32', C.byref(self.c), rot6d, shape, gt_vert, gt_joint, gt_rot6d, gt_shape, is_right, is_ho3d, bs, weights[0],
              weights[1], weights[2], weights[3], d6, ds, parts, verts, joints)
        tot = parts.sum(0)
        L = dict(vert_loss=tot[0] * (weights[0] / (bs * 2334.0)), joint_loss=tot[1] * (weights[1] / (bs * 63.0)),
                 mano_pose_loss=tot[2] * (weights[2] / (bs * 96.0)), mano_shape_loss=tot[3] * (weights[3] / (bs * 10.0)))
        return (L, d6, ds, verts, joints) if want_outputs else (L, d6, ds)

    def fk(self, pose, shape_ctx, hands_per_image, want_verts=True, ho3d=None):
        """pose (n, >=48) rows; shape_ctx = self.shape(betas).  -> verts (n,778,3)|None, joints (n,21,3)"""
        n, ld = pose.shape
        vs, J = shape_ctx
        verts = _new((n, 778, 3), pose) if want_verts else None
        joints = _new((n, 21, 3), pose)
        _call('vpho_mano_fk_f32', C.byref(self.c), pose, ld, n, hands_per_image, vs, J, ho3d, verts, joints)
        return verts, joints


# ----------------------------------------------------------------------------------------------- aggregation
ObjTables = abi.struct('vpho_obj_tables')
AnchorTables = abi.struct('vpho_anchor_tables')
HandSurfaceTable = abi.struct('vpho_hand_surface_table')


class HandSurface:
    """Vertex normals of a posed hand mesh + the finger-gap fill (csrc/hand_surface.hip; base.py:887-891, hand_fn.py:294-384).

    ``HandSurface(faces, links, alpha, device, n_verts=None)``: faces (F,3), links (L,2) integer arrays, alpha (L,) float64; ``n_verts``
    (default: the largest index + 1) lets a mesh end in unreferenced vertices.  Every index is validated HERE, once: the kernel trusts the
    table.  ``fill(verts (n,V,3)) -> verts_filled, normals_filled (n,V+L,3)``."""
    MAX_V, MAX_F, MAX_L = 1024, 2048, 1024

    def __init__(self, faces, links, alpha, device, n_verts=None):
        import numpy as np
        faces = np.asarray(faces).reshape(-1, 3)
        links = np.asarray(links).reshape(-1, 2)
        alpha = np.asarray(alpha, np.float64).reshape(-1)
        if faces.dtype.kind not in 'iu' or links.dtype.kind not in 'iu':
            raise VphoError(f'HandSurface: faces and links must be integer arrays, got {faces.dtype} and {links.dtype}')
        faces, links = faces.astype(np.int64), links.astype(np.int64)
        top = max(int(faces.max()) if faces.size else -1, int(links.max()) if links.size else -1)
        V = int(n_verts) if n_verts is not None else top + 1
        Fn, L = len(faces), len(links)
        if not 1 <= V <= self.MAX_V:
            raise VphoError(f'HandSurface: {V} vertices, the kernel takes 1 .. {self.MAX_V}')
        if Fn > self.MAX_F:
            raise VphoError(f'HandSurface: {Fn} faces, the kernel takes at most {self.MAX_F}')
        if L > self.MAX_L:
            raise VphoError(f'HandSurface: {L} links, the kernel takes at most {self.MAX_L}')
        if len(alpha) != L:
            raise VphoError(f'HandSurface: {L} links with {len(alpha)} weights')
        for name, a in (('face', faces), ('link', links)):
            if a.size and (a.min() < 0 or a.max() >= V):
                bad = int(np.flatnonzero(((a < 0) | (a >= V)).any(1))[0])
                raise VphoError(f'HandSurface: {name} {bad} = {a[bad].tolist()} indexes outside the {V} vertices')
        if not np.isfinite(alpha).all():
            raise VphoError('HandSurface: a link weight is not finite')
        # vertex -> (face, corner), the faces of a vertex in ascending index (a stable sort of the face-major corner list)
        flat = faces.reshape(-1)
        order = np.argsort(flat, kind='stable')
        entry = (order // 3) * 4 + order % 3
        offset = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=V))])
        dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a).astype(dt)).to(device).contiguous()
        # an empty array still needs an address the structure can hold
        self.faces, self.csr_offset, self.csr_entry = dev(faces, np.int32), dev(offset, np.int32), dev(entry, np.int32)
        self.links, self.alpha = dev(links, np.int32), dev(alpha, np.float64)
        self.V, self.F, self.L, self.device = V, Fn, L, device
        self.table = HandSurfaceTable(*[t.data_ptr() if t.numel() else None for t in (self.faces, self.csr_offset, self.csr_entry, self.links, self.alpha)],
                                      V, Fn, L)

    def fill(self, verts, out=None):
        if verts.dim() != 3 or tuple(verts.shape[1:]) != (self.V, 3):
            raise VphoError(f'HandSurface.fill: verts of shape {tuple(verts.shape)}, the table was built for (n, {self.V}, 3)')
        n = verts.shape[0]
        vf, nf = out if out is not None else (_new((n, self.V + self.L, 3), verts), _new((n, self.V + self.L, 3), verts))
        if any(tuple(t.shape) != (n, self.V + self.L, 3) for t in (vf, nf)):
            raise VphoError(f'HandSurface.fill: outputs of shape {tuple(vf.shape)} and {tuple(nf.shape)}, expected {(n, self.V + self.L, 3)}')
        _call('vpho_hand_surface_f32', C.byref(self.table), verts, n, vf, nf)
        return vf, nf


def _ids_to_device(ids, device):
    host = torch.tensor(ids, dtype=torch.int32).pin_memory()        # the caching host allocator keeps the block until the copy's event
    return host.to(device, non_blocking=True)


class Aggregation:
    """Device tables + thin wrappers of the aggregation kernels."""

    def __init__(self, assets, anchor_skeleton, device):
        ycb = assets['ycb']
        self.names = list(ycb.keys())
        self.name_to_id = {n: i for i, n in enumerate(self.names)}
        f = lambda a: torch.as_tensor(a, dtype=torch.float32).to(device).contiguous()
        stack = lambda key: torch.stack([torch.as_tensor(ycb[n][key], dtype=torch.float32).reshape(-1, 3) for n in self.names]).to(device).contiguous()
        self.kpt, self.vert = stack('kpt3d'), stack('verts_sampled')
        self.com = stack('CoM').reshape(len(self.names), 3).contiguous()
        self.obj = ObjTables(self.kpt.data_ptr(), self.vert.data_ptr(), self.com.data_ptr(), self.kpt.shape[1], self.vert.shape[1], len(self.names))
        a = assets['anchor']
        self.face = torch.as_tensor(a['face_vert_idx'], dtype=torch.int32).to(device).contiguous()
        self.aw = f(a['anchor_weight'])
        self.v2j = f(a['vert2joint'])
        self.skel = torch.as_tensor(anchor_skeleton, dtype=torch.int32).to(device).contiguous()
        self.anchor = AnchorTables(self.face.data_ptr(), self.aw.data_ptr(), self.v2j.data_ptr(), self.skel.data_ptr())
        self.device = device

    def obj_ids(self, names):
        """class indices of a batch as a device tensor: filled into pinned host memory and copied asynchronously on the CALLER's current
        stream, every call (a pageable-memory copy would park the calling thread behind everything queued on its stream; a cache shared
        by the evaluator's slot threads would hand a tensor allocated on one stream to kernels of another -- ADVICE r3)"""
        return _ids_to_device([self.name_to_id[n] for n in names], self.device)

    def hand_candidates(self, diff_pose, reg_pose, bs, S):
        pose = _new((bs, 2 * S, 48), diff_pose)
        _call('vpho_hand_candidates_f32', diff_pose, diff_pose.shape[-1], reg_pose, bs, S, pose)
        return pose

    def hand_heat(self, joints, root, K, bbox, heatmap, observe):
        bs, Cn = joints.shape[:2]
        _, J, H, W = heatmap.shape
        out = _new((bs, Cn, len(observe)), joints)
        obs = (C.c_int * len(observe))(*observe)
        _call('vpho_hand_heat_f32', joints, root, K, bbox, heatmap, bs, Cn, J, H, W, obs, len(observe), out)
        return out

    def hand_fuse_level(self, hv, pose, k, level, want_topk_pose=False, want_scores=False):
        bs, Cn, n_obs = hv.shape
        Fn = 1 if level == 0 else 5
        val, idx = _new((bs, Fn, k), hv), _new((bs, Fn, k), hv, torch.int32)
        tp = _new((bs, k, Fn, 3), hv) if want_topk_pose else None
        sc = _new((bs, Cn, Fn), hv) if want_scores else None
        _call('vpho_hand_fuse_level_f32', hv, n_obs, pose, bs, Cn, k, level, val, idx, tp, sc)
        return (val, idx, tp, sc) if want_scores else (val, idx, tp)

    def topk(self, scores, k, F_=1):
        """scores (rows, n) [F_=1] or (rows, n, F_) -> val, idx (rows, F_, k)"""
        rows, n = scores.shape[:2]
        val, idx = _new((rows, F_, k), scores), _new((rows, F_, k), scores, torch.int32)
        _call('vpho_topk_f32', scores, rows, n, F_, k, val, idx)
        return val, idx

    def topk_weights(self, val):
        w = torch.empty_like(val)
        _call('vpho_topk_weights_f32', val, val.numel() // val.shape[-1], val.shape[-1], w)
        return w

    def obj_heat_score(self, pose, root, obj_id, is_right, K, bbox, heatmap, transl_override=None):
        bs, n = pose.shape[:2]
        _, J, H, W = heatmap.shape
        assert J == self.obj.n_kpt
        score = _new((bs, n), root)
        _call('vpho_obj_heat_score', pose, n, transl_override, root, C.byref(self.obj), obj_id, is_right, K, bbox, heatmap, bs, H, W, score)
        return score

    def obj_cross(self, pose, transl_idx, rot_idx):
        bs, n = pose.shape[:2]
        ko = transl_idx.shape[-1]
        cand = _new((bs, ko * ko, 9), pose, torch.float64)
        _call('vpho_obj_cross_candidates', pose, n, transl_idx, rot_idx, bs, ko, cand)
        return cand

    def obj_physics_score(self, cand, root, obj_id, is_right, force_point, force_global):
        bs, n = cand.shape[:2]
        score = _new((bs, n), root)
        _call('vpho_obj_physics_score', cand, n, root, C.byref(self.obj), obj_id, is_right, force_point, force_global, bs, score)
        return score

    def obj_fuse(self, pose, idx_a, w_a, idx_b=None, w_b=None, pick_b=None):
        bs, n = pose.shape[:2]
        k = idx_a.shape[-1]
        fused = _new((bs, 9), pose, torch.float64)
        _call('vpho_obj_fuse_f64', pose, n, idx_a, w_a, idx_b, w_b, pick_b, bs, k, fused)
        return fused

    def obj_verts(self, pose, root, obj_id, is_right):
        bs = pose.shape[0]
        out = _new((bs, self.obj.n_vert, 3), root)
        _call('vpho_obj_verts_f32', pose, root, C.byref(self.obj), obj_id, is_right, bs, out)
        return out

    def force_anchor(self, verts, root, force_local_, hands_per_image):
        n = verts.shape[0]
        fp, fg = _new((n, 32, 3), verts), _new((n, 32, 3), verts)
        _call('vpho_force_anchor_f32', C.byref(self.anchor), verts, root, force_local_, n, hands_per_image, fp, fg)
        return fp, fg

    def contact_detect(self, hand_verts, hand_normals, obj_verts, obj_normals, normal_thresh=(-0.015, 0.01), vertical_thresh=0.01,
                       decay=(-0.005, 0.005)):
        """detect_hand_and_object_contact (physics_fn.py:47-117) for n samples: (n,Nh,3), (n,Nh,3), (n,No,3), (n,No,3) ->
        hand_contact (n,Nh), obj_contact (n,No), obj_contact_to_hand_vert (n,No) int32"""
        n, nh, _ = hand_verts.shape
        no = obj_verts.shape[1]
        hc, oc = _new((n, nh), hand_verts), _new((n, no), hand_verts)
        o2h = _new((n, no), hand_verts, torch.int32)
        (n0, n1), v, (d0, d1) = normal_thresh, vertical_thresh, decay
        _call('vpho_contact_detect_f32', hand_verts, hand_normals, obj_verts, n, nh, no, n0, n1, v, d0, d1, hc, None)
        _call('vpho_contact_detect_f32', obj_verts, obj_normals, hand_verts, n, no, nh, n0, n1, v, d0, d1, oc, o2h)
        return hc, oc, o2h

    def hand_contact(self, hand_verts, hand_normals, obj_verts, normal_thresh=(-0.015, 0.01), vertical_thresh=0.01, decay=(-0.005, 0.005)):
        """the hand -> object half of detect_hand_and_object_contact, all that get_hand_contact keeps (base.py:898-911): (n,Nh,3), (n,Nh,3),
        (n,No,3) -> hand_contact (n,Nh); one launch, no object normals"""
        n, nh, _ = hand_verts.shape
        hc = _new((n, nh), hand_verts)
        _call('vpho_contact_detect_f32', hand_verts, hand_normals, obj_verts, n, nh, obj_verts.shape[1], normal_thresh[0], normal_thresh[1],
              vertical_thresh, decay[0], decay[1], hc, None)
        return hc

    def force_contact(self, hand_contact, thresh=0.0):
        """ForceAnchor.get_force_contact + check_is_grasped (physics_fn.py:201-221): (n, >=778) -> (n,32), (n,) uint8"""
        n, ld = hand_contact.shape
        fc, gr = _new((n, 32), hand_contact), _new((n,), hand_contact, torch.uint8)
        _call('vpho_force_contact_f32', C.byref(self.anchor), hand_contact, ld, n, thresh, fc, gr)
        return fc, gr

    def anchor_frames(self, verts):
        """ForceAnchor.__call__ (physics_fn.py:224-257): verts (n,778,3) -> points (n,32,3), frames (n,32,3,3)"""
        n = verts.shape[0]
        pts, frames = _new((n, 32, 3), verts), _new((n, 32, 3, 3), verts)
        _call('vpho_anchor_frames_f32', C.byref(self.anchor), verts, n, pts, frames)
        return pts, frames

    def force_optimize(self, verts, gravity, com, force_contact, is_grasped, batch_size, iters=3000, phase1=300, lr=1e-3):
        """ForceOptimizer.optimize_batch inner loop (force_optimization.py:110-207) for n = n_batches*batch_size samples."""
        n = verts.shape[0]
        assert n % batch_size == 0, 'pad the last batch: the batch-mean force loss couples the samples of a batch'
        pts, frames = self.anchor_frames(verts)
        fl, fg = _new((n, 32, 3), verts), _new((n, 32, 3), verts)
        scale, weight, losses = _new((n, 32), verts), _new((n, 32, 8), verts), _new((n // batch_size, 4), verts)
        _call('vpho_force_optimize_f32', pts, frames, gravity, com, force_contact, is_grasped, n // batch_size, batch_size, iters, phase1, lr, fl,
              fg, scale, weight, losses)
        return dict(force_local=fl, force_global=fg, scale=scale, weight=weight, losses=losses, force_point=pts, frames=frames)

    def hand_phys_candidates(self, agg_pose, betas, topk_pose):
        bs, k = topk_pose.shape[:2]
        out = _new((bs, k + 1, 58), agg_pose)
        _call('vpho_hand_phys_candidates_f32', agg_pose, agg_pose.shape[-1], betas, topk_pose, bs, k, out)
        return out

    def hand_phys_score(self, force_point, force_global, obj_vert, bs, n_cand):
        out = _new((bs, n_cand, 5), force_point)
        _call('vpho_hand_phys_score_f32', force_point, force_global, obj_vert, obj_vert.shape[1], bs, n_cand, out)
        return out

    def hand_phys_fuse(self, cand, idx):
        bs, n_cand = cand.shape[:2]
        out = _new((bs, 58), cand)
        _call('vpho_hand_phys_fuse_f32', cand, n_cand, idx, bs, idx.shape[-1], out)
        return out

    # ---- the ablation aggregators (aggregation modes other than heatmap_cascade; csrc/aggregate_modes.hip)
    def heatmap_peak(self, heatmap):
        """heatmap (bs,J,H,W) -> peak (bs,J,2) in the reference's transposed (-1, 1) grid, flat arg-max index (bs,J) int32"""
        bs, J, H, W = heatmap.shape
        peak, ind = _new((bs, J, 2), heatmap), _new((bs, J), heatmap, torch.int32)
        _call('vpho_heatmap_peak_f32', heatmap, bs * J, H, W, peak, ind)
        return peak, ind

    def hand_pt2d_score(self, joints, root, K, bbox, peak, per_joint=False):
        """joints (bs,C,21,3), peak (bs,21,2) -> (bs,C) or, per_joint, (bs,C,21)"""
        bs, Cn = joints.shape[:2]
        score = _new((bs, Cn, 21) if per_joint else (bs, Cn), joints)
        _call('vpho_hand_pt2d_score_f32', joints, root, K, bbox, peak, bs, Cn, int(per_joint), score)
        return score

    def obj_pt2d_score(self, pose, root, obj_id, is_right, K, bbox, peak):
        bs, n = pose.shape[:2]
        assert peak.shape[1] == self.obj.n_kpt
        score = _new((bs, n), root)
        _call('vpho_obj_pt2d_score', pose, n, root, C.byref(self.obj), obj_id, is_right, K, bbox, peak, bs, score)
        return score

    def hand_pose_fuse(self, pose, idx=None, w=None, n=None):
        """pose (bs,C,>=48) rows; idx / w (bs,n) or None (candidates 0 .. n-1 / unweighted) -> fused axis-angle (bs,48)"""
        bs, Cn, ld = pose.shape
        n = idx.shape[-1] if idx is not None else (Cn if n is None else n)
        fused = _new((bs, 48), pose)
        _call('vpho_hand_pose_fuse_f32', pose, ld, Cn, idx, w, bs, n, fused)
        return fused

    def hand_joint_gather_mean(self, joints, idx):
        """joints (bs,C,21,3), idx (bs,21,k) -> (bs,21,3)"""
        bs, Cn = joints.shape[:2]
        fused = _new((bs, 21, 3), joints)
        _call('vpho_hand_joint_gather_mean_f32', joints, idx, bs, Cn, idx.shape[-1], fused)
        return fused


# ----------------------------------------------------------------------------------------------- metrics
def hand_metrics(pd, gt, per_point=False):
    """pd, gt (n,P,3) fp32 metres -> mean error (n,), Procrustes-aligned mean error (n,), [per-point errors (n,P)]
    (test.py:657-680)."""
    n, P, _ = pd.shape
    assert gt.shape == pd.shape
    me, pa = _new((n,), pd), _new((n,), pd)
    pp = _new((n, P), pd) if per_point else None
    _call('vpho_hand_metrics_f32', pd, gt, n, P, me, pa, pp)
    return (me, pa, pp) if per_point else (me, pa)


def hand_metrics_multi(pd, gt, root_joint, is_right):
    """Every sampled hand hypothesis against the image's ground truth (TesterHand.__call__ on pd (n,S,P,3), test.py:589-597,657-679).
    pd (n,S,P,3) fp32 in the model frame as predict returns it (diff_final_hand_joint / _vert); the postprocess of
    train_diff_hand_obj.py:578-602 (un-flip x of left hands, add the root) happens in the kernel as points are loaded.
    gt (n,P,3) fp32, root_joint (n,3) fp32, is_right (n,) bool -> MJE (n,S), PA-MJE (n,S) in metres."""
    n, S, P, _ = pd.shape
    assert gt.shape == (n, P, 3) and root_joint.shape == (n, 3) and is_right.shape == (n,)
    me, pa = _new((n, S), pd), _new((n, S), pd)
    flag = is_right.to(device=pd.device, dtype=torch.uint8).contiguous()
    _call('vpho_hand_metrics_multi_f32', pd, gt, root_joint, flag, n, S, P, me, pa)
    return me, pa


HAND_BENCH_MAX_POINTS = 1024            # csrc/hand_bench.hip: three point sets of a pair in LDS
_HAND_BENCH_TABLES = {}


def hand_bench_tables(device):
    """the AUC threshold table t = np.linspace(*HAND_BENCH_AUC) (n_t,) fp64 and G (n_t + 1,) fp64 on ``device``, built once per device:
    G[c] = the trapezoid integral over the table of the step 1[e <= t] of a point with c = #{j : e <= t_j}, divided by t[-1] - t[0];
    with j0 = n_t - c: ((t[-1] - t[j0]) + (t[j0] - t[j0 - 1]) / 2 if j0 >= 1) / (t[-1] - t[0]), G[0] = 0"""
    key = str(torch.device(device))
    if key not in _HAND_BENCH_TABLES:
        import numpy as np
        from .ops_names import HAND_BENCH_AUC
        t = np.linspace(HAND_BENCH_AUC[0], HAND_BENCH_AUC[1], HAND_BENCH_AUC[2])
        n_t = t.shape[0]
        g = np.zeros(n_t + 1)
        for c in range(1, n_t + 1):
            j0 = n_t - c
            g[c] = ((t[-1] - t[j0]) + ((t[j0] - t[j0 - 1]) / 2 if j0 >= 1 else 0.0)) / (t[-1] - t[0])
        _HAND_BENCH_TABLES[key] = (torch.from_numpy(t).to(device), torch.from_numpy(g).to(device))
    return _HAND_BENCH_TABLES[key]


def hand_bench_multi(pd, gt, root_joint, is_right, with_fscore=True, counts=False):
    """The hand leaderboard values of every sampled hypothesis (FreiHAND / HO3D eval.py).  pd (n,S,P,3) fp32 in the
    model frame as predict returns it (the postprocess happens on load, as in hand_metrics_multi), gt (n,P,3), root_joint (n,3),
    is_right (n,) -> values (n,S,6) fp64 = AUC, PA AUC of the PCK curve over ops_names.HAND_BENCH_AUC, then F, F, PA F, PA F at the two
    ops_names.HAND_BENCH_F_THRESH (NaN without ``with_fscore``: the joint call); with ``counts`` also (n,S,10) int32: the eight
    nearest-neighbour counts {raw, PA} x {d1, d2} x {lo, hi}, then the sums of the AUC counts raw and aligned.  A pair with a
    non-finite coordinate is NaN.  S = 1 serves a single hand per image: ``out['agg_hand_vert'][:, None]``."""
    from .ops_names import HAND_BENCH_F_THRESH
    n, S, P, _ = pd.shape
    assert pd.shape == (n, S, P, 3) and gt.shape == (n, P, 3) and root_joint.shape == (n, 3) and is_right.shape == (n,)
    if P > HAND_BENCH_MAX_POINTS or P < 3:
        raise VphoError(f'hand_bench_multi: {P} points per hand, the kernel takes 3 .. {HAND_BENCH_MAX_POINTS}')
    if n * S > 0x7fffffff:
        raise VphoError(f'hand_bench_multi: {n} x {S} pairs, at most 2^31 - 1 in one call')
    values = _new((n, S, 6), pd, torch.float64)
    cnt = _new((n, S, 10), pd, torch.int32) if counts else None
    if n * S > 0:
        t, g = hand_bench_tables(pd.device)
        flag = is_right.to(device=pd.device, dtype=torch.uint8).contiguous()
        _call('vpho_hand_bench_multi_f32', pd, gt, root_joint, flag, n, S, P, HAND_BENCH_F_THRESH[0], HAND_BENCH_F_THRESH[1], t, g, t.shape[0],
              1 if with_fscore else 0, values, cnt if counts else None)
    return (values, cnt) if counts else values


def hand_bench_table(per):
    """per (n,S,8) fp64 in the order of ops_names.HAND_BENCH_NAMES -> one, best, mean, each (n,8) fp64: hypothesis 0, the per-value
    MAXIMUM over the S hypotheses, the mean (fp64 sum in ascending s); a NaN hypothesis makes best and mean NaN"""
    n, S, k = per.shape
    assert k == 8 and S > 0
    one, best, mean = (_new((n, 8), per, torch.float64) for _ in range(3))
    if n > 0:
        _call('vpho_hand_bench_table_f64', per, n, S, one, best, mean)
    return one, best, mean


def obj_9d_to_rt(pose9, root_joint):
    """(n,9) fp64 [rot6d | t], (n,3) fp32 root -> (n,3,4) fp64 [R | t + root]  (transform_fn.py:85-90, train_diff_hand_obj.py:594-597)"""
    n = pose9.shape[0]
    rt = _new((n, 3, 4), pose9, torch.float64)
    _call('vpho_obj_9d_to_rt_f64', pose9, root_joint, n, rt)
    return rt


def infer_record_dtype(n_joint=21, n_vert=778):
    """numpy structured dtype of one vpho_infer_pack_f32 record (include/vpho_hip.h): blocks A (fp32), B (fp16), C (fp64)"""
    import numpy as np
    size = abi.query('vpho_infer_record_bytes', n_joint, n_vert)
    if size < 0:
        raise VphoError(f'vpho_infer_record_bytes: n_joint = {n_joint}, n_vert = {n_vert} (both positive, n_vert even)')
    a = 24 * (n_joint + n_vert)
    return np.dtype({'names': ['reg_joint', 'reg_vert', 'agg_joint', 'agg_vert', 'agg_vert_f16', 'pd_obj_rt'],
                     'formats': [('<f4', (n_joint, 3)), ('<f4', (n_vert, 3)), ('<f4', (n_joint, 3)), ('<f4', (n_vert, 3)), ('<f2', (n_vert, 3)),
                                 ('<f8', (3, 4))],
                     'offsets': [0, 12 * n_joint, 12 * (n_joint + n_vert), 12 * (2 * n_joint + n_vert), a, size - 96], 'itemsize': size})


class InferPacker:
    """Prediction records of --mode infer (vpho_infer_pack_f32): per slot of the evaluation pipeline a device staging buffer and a PINNED
    host buffer of ``max_batch`` records.  ``pack`` = one kernel launch + one hipMemcpyAsync on the caller's stream + one event;
    ``collect`` waits for that event only and returns the records as a numpy view of the pinned buffer (valid until the slot's next
    ``pack``).  Nothing here synchronises the device."""

    def __init__(self, device, max_batch, slots=3, n_joint=21, n_vert=778):
        self.device, self.max_batch, self.slots = torch.device(device), int(max_batch), int(slots)
        self.n_joint, self.n_vert = n_joint, n_vert
        self.dtype = infer_record_dtype(n_joint, n_vert)
        self.record_bytes = self.dtype.itemsize
        self.stage = [torch.empty(self.max_batch * self.record_bytes, dtype=torch.uint8, device=self.device) for _ in range(self.slots)]
        self.host = [torch.empty(self.max_batch * self.record_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(self.slots)]
        self.events = [None] * self.slots
        self.counts = [0] * self.slots

    def pack(self, out, batch, stream=None, slot=0):
        """out: the predict outputs; batch: its 'root_joint' (n,3) and 'is_right' (n,), on the device.  Enqueued on ``stream`` (default: the
        current one).  Returns the slot."""
        n = out['agg_hand_joint'].shape[0]
        if n > self.max_batch:
            raise VphoError(f'InferPacker.pack: a batch of {n} images, the packer was built for max_batch = {self.max_batch}')
        if not 0 <= slot < self.slots:
            raise VphoError(f'InferPacker.pack: slot {slot} of {self.slots}')
        stream = torch.cuda.current_stream(self.device) if stream is None else stream
        c = lambda t: t.float().contiguous()
        J, V = self.n_joint, self.n_vert
        rj, rv, aj, av = c(out['reg_hand_joint']), c(out['reg_hand_vert']), c(out['agg_hand_joint']), c(out['agg_hand_vert'])
        if rj.shape != (n, J, 3) or aj.shape != (n, J, 3) or rv.shape != (n, V, 3) or av.shape != (n, V, 3):
            raise VphoError(f'InferPacker.pack: hand arrays {tuple(rj.shape)} {tuple(rv.shape)} {tuple(aj.shape)} {tuple(av.shape)}, expected (n,{J},3) / (n,{V},3)')
        o9 = out['agg_obj_6d'].double().contiguous()
        root = c(batch['root_joint'])
        flag = batch['is_right']
        # a bool tensor on the device is read as it stands (one byte per image, 0 / 1): no conversion launch
        flag = flag.contiguous().view(torch.uint8) if flag.is_cuda and flag.dtype == torch.bool else flag.to(device=self.device, dtype=torch.uint8).contiguous()
        if o9.shape != (n, 9) or root.shape != (n, 3) or flag.shape != (n,):
            raise VphoError(f'InferPacker.pack: agg_obj_6d {tuple(o9.shape)}, root_joint {tuple(root.shape)}, is_right {tuple(flag.shape)} for {n} images')
        with torch.cuda.stream(stream):
            _call('vpho_infer_pack_f32', rj, rv, aj, av, o9, root, flag, n, J, V, self.stage[slot], C.c_void_p(self.host[slot].data_ptr()))
            ev = torch.cuda.Event(blocking=True)
            ev.record(stream)
        self.events[slot], self.counts[slot] = ev, n
        return slot

    def collect(self, slot):
        """the records of the slot's last ``pack`` (numpy, ``self.dtype``, a VIEW of the pinned buffer) once its copy has landed"""
        if self.events[slot] is None:
            raise VphoError(f'InferPacker.collect: nothing was packed into slot {slot}')
        self.events[slot].synchronize()
        return self.host[slot].numpy()[:self.counts[slot] * self.record_bytes].view(self.dtype)


ObjMetricTables = abi.struct('vpho_obj_metric_tables')


from .ops_names import OBJ_METRIC_NAMES  # noqa: E402,F401


class ObjectMetrics:
    """TesterObject (lib/engine/test.py:240-503) on the device: fp64 model tables + thin wrapper of vpho_obj_metrics_f64."""

    def __init__(self, ycb, device):
        import numpy as np
        self.names = list(ycb.keys())
        self.name_to_id = {n: i for i, n in enumerate(self.names)}
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)
        self.bbox3d = d(np.stack([np.asarray(ycb[n]['bbox3d']).reshape(8, 3) for n in self.names]))
        self.verts_sampled = d(np.stack([np.asarray(ycb[n]['verts_sampled']).reshape(-1, 3) for n in self.names]))
        counts = [int(np.asarray(ycb[n]['verts']).reshape(-1, 3).shape[0]) for n in self.names]
        self.max_verts = max(counts)
        self.verts = d(np.concatenate([np.asarray(ycb[n]['verts']).reshape(-1, 3) for n in self.names]))
        self.vert_offset = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(device)
        self.diameter = d(np.array([float(ycb[n]['diameter']) for n in self.names]))
        self.c = ObjMetricTables(self.bbox3d.data_ptr(), self.verts_sampled.data_ptr(), self.verts.data_ptr(),
                                 self.vert_offset.data_ptr(), self.diameter.data_ptr(), len(self.names), self.verts_sampled.shape[1])
        self.device = device

    def obj_ids(self, names):
        """class indices of a batch as a device tensor: filled into pinned host memory and copied asynchronously on the CALLER's current
        stream, every call (a pageable-memory copy would park the calling thread behind everything queued on its stream; a cache shared
        by the evaluator's slot threads would hand a tensor allocated on one stream to kernels of another -- ADVICE r3)"""
        return _ids_to_device([self.name_to_id[n] for n in names], self.device)

    def __call__(self, pd_rt, gt_rt, cam_intr, obj_id):
        """pd_rt, gt_rt (n,3,4), cam_intr (n,3,3) fp64, obj_id (n,) int32 -> (n,16) fp64 in the order of OBJ_METRIC_NAMES."""
        n = pd_rt.shape[0]
        assert gt_rt.shape == (n, 3, 4) and pd_rt.shape == (n, 3, 4) and cam_intr.shape == (n, 3, 3) and obj_id.shape == (n,)
        need = abi.query('vpho_obj_metrics_workspace_bytes', C.byref(self.c), n, self.max_verts)
        if need < 0:
            raise VphoError('vpho_obj_metrics_workspace_bytes: bad argument')
        # a fresh block from torch's caching allocator per call (stream-ordered reuse): one object serves the evaluator's slots, whose
        # streams run concurrently -- a workspace kept on the object would be shared by kernels of different streams
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = _new((n, 16), pd_rt, torch.float64)
        _call('vpho_obj_metrics_f64', C.byref(self.c), pd_rt, gt_rt, cam_intr, obj_id, n, self.max_verts, out, ws, ws.numel())
        return out

    def multi(self, pd_rt, gt_rt, cam_intr, obj_id):
        """Every sampled object hypothesis (TesterObject.__call__ per candidate slice pd_rt[:, s], then TesterObject.postprocess,
        test.py:240-567).  pd_rt (n,S,3,4), gt_rt (n,3,4), cam_intr (n,3,3) fp64, obj_id (n,) int32 ->
        per-candidate (n,S,16), best-of-S (n,16) and mean-of-S (n,16) fp64, columns in the order of OBJ_METRIC_NAMES."""
        n, S = pd_rt.shape[:2]
        assert pd_rt.shape == (n, S, 3, 4) and gt_rt.shape == (n, 3, 4) and cam_intr.shape == (n, 3, 3) and obj_id.shape == (n,)
        need = abi.query('vpho_obj_metrics_multi_workspace_bytes', C.byref(self.c), n, S, self.max_verts)
        if need < 0:
            raise VphoError('vpho_obj_metrics_multi_workspace_bytes: bad argument')
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)          # per call, as in __call__
        per, best, mean = _new((n, S, 16), pd_rt, torch.float64), _new((n, 16), pd_rt, torch.float64), _new((n, 16), pd_rt, torch.float64)
        _call('vpho_obj_metrics_multi_f64', C.byref(self.c), pd_rt, gt_rt, cam_intr, obj_id, n, S, self.max_verts, per, best, mean, ws, ws.numel())
        return per, best, mean


ObjSymmetryTables = abi.struct('vpho_obj_symmetry_tables')


SYMMETRY_MAX_TRANSFORMS = 4096           # vpho_obj_symmetry_multi_f64: symmetry transforms per object


class ObjectSymmetry:
    """The symmetry-aware object errors (--eval_symmetric) on the device: SMCE (TesterObject.criterion_SMCE,
    lib/engine/test.py:377-398), MSSD and MSSD < 0.1 * diameter over a padded symmetry table.  ``ycb``: {name: {'bbox3d' (8, 3),
    'verts_sampled' (P, 3), 'diameter'}} with one P >= 1 for all; ``table``: (R (n_obj, K, 3, 3), t (n_obj, K, 3)) in the order of
    ``ycb`` (symmetry.symmetry_table).  ``prune`` (default on) lets the kernel abandon a symmetry that can no longer be the minimum; both
    settings return the same bits."""

    def __init__(self, ycb, table, device, prune=True):
        import numpy as np
        self.names = list(ycb.keys())
        self.name_to_id = {n: i for i, n in enumerate(self.names)}
        R, t = (np.ascontiguousarray(a, dtype=np.float64) for a in table)
        if R.ndim != 4 or R.shape[0] != len(self.names) or R.shape[2:] != (3, 3) or t.shape != R.shape[:2] + (3,) or R.shape[1] < 1:
            raise VphoError(f'ObjectSymmetry: table R {R.shape} / t {t.shape} for {len(self.names)} objects, expected (n_obj, K, 3, 3) / (n_obj, K, 3)')
        if R.shape[1] > SYMMETRY_MAX_TRANSFORMS:
            raise VphoError(f'ObjectSymmetry: {R.shape[1]} symmetry transforms per object, at most {SYMMETRY_MAX_TRANSFORMS} (a larger '
                            f'--max_sym_disc_step gives a shorter table)')
        if not torch.device(device).type == 'cuda':
            raise VphoError('vpho_amd ops take GPU tensors only (no CPU path)')
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)
        self.sym_R, self.sym_t = d(R), d(t)
        self.bbox3d = d(np.stack([np.asarray(ycb[n]['bbox3d']).reshape(8, 3) for n in self.names]))
        self.verts_sampled = d(np.stack([np.asarray(ycb[n]['verts_sampled']).reshape(-1, 3) for n in self.names]))
        self.diameter = d(np.array([float(ycb[n]['diameter']) for n in self.names]))
        self.K, self.prune, self.device = int(R.shape[1]), bool(prune), device
        self.c = ObjSymmetryTables(self.sym_R.data_ptr(), self.sym_t.data_ptr(), self.bbox3d.data_ptr(), self.verts_sampled.data_ptr(),
                                   self.diameter.data_ptr(), self.K, len(self.names), self.verts_sampled.shape[1])

    def obj_ids(self, names):
        """class indices of a batch as a device tensor (ObjectMetrics.obj_ids)"""
        return _ids_to_device([self.name_to_id[n] for n in names], self.device)

    def _check_ids(self, obj_id, n):
        """obj_id as an (n,) device tensor: a host sequence of ints is range-checked and copied (a device tensor cannot be refused without
        a host sync: the kernel gives NaN, NaN, 0 for an id outside the table)"""
        if not torch.is_tensor(obj_id):
            ids = [int(i) for i in obj_id]
            if len(ids) != n or any(i < 0 or i >= len(self.names) for i in ids):
                raise VphoError(f'ObjectSymmetry: object ids {ids} outside [0, {len(self.names)}) or not one per image')
            obj_id = _ids_to_device(ids, self.device)
        if obj_id.shape != (n,):
            raise VphoError(f'ObjectSymmetry: obj_id {tuple(obj_id.shape)} for {n} images')
        return obj_id

    def per_hypothesis(self, pd_rt, gt_rt, obj_id, prune=None):
        """pd_rt (n, S, 3, 4), gt_rt (n, 3, 4) fp64, obj_id (n,) int32 device tensor or host ints -> (n, S, 3) fp64 = SMCE (m), MSSD (m),
        MSSD < 0.1 * diameter; a fresh output block per call (stream-ordered, as ObjectMetrics' workspace), no workspace"""
        n, S = pd_rt.shape[:2]
        if pd_rt.shape != (n, S, 3, 4) or gt_rt.shape != (n, 3, 4):
            raise VphoError(f'ObjectSymmetry: pd_rt {tuple(pd_rt.shape)}, gt_rt {tuple(gt_rt.shape)}, expected (n, S, 3, 4) and (n, 3, 4)')
        if not (pd_rt.is_cuda and gt_rt.is_cuda):
            raise VphoError('vpho_amd ops take GPU tensors only (no CPU path)')
        obj_id = self._check_ids(obj_id, n)
        per = _new((n, S, 3), pd_rt, torch.float64)
        _call('vpho_obj_symmetry_multi_f64', C.byref(self.c), pd_rt, gt_rt, obj_id, n, S, int(self.prune if prune is None else prune), per)
        return per

    def __call__(self, pd_rt, gt_rt, obj_id, prune=None):
        """one pose per image: pd_rt, gt_rt (n, 3, 4) -> (n, 3) in the order of ops_names.SYM_METRIC_NAMES (the S = 1 launch)"""
        if pd_rt.dim() != 3:
            raise VphoError(f'ObjectSymmetry: pd_rt {tuple(pd_rt.shape)}, expected (n, 3, 4)')
        return self.per_hypothesis(pd_rt[:, None], gt_rt, obj_id, prune)[:, 0]

    def multi(self, pd_rt, gt_rt, obj_id, prune=None):
        """every sampled hypothesis: -> per (n, S, 3), best-of-S (n, 3: min SMCE, min MSSD, max hit), mean-of-S (n, 3)"""
        per = self.per_hypothesis(pd_rt, gt_rt, obj_id, prune)
        n, S = per.shape[:2]
        one, best, mean = (_new((n, 3), per, torch.float64) for _ in range(3))
        _call('vpho_obj_symmetry_table_f64', per, n, S, one, best, mean)
        return per, best, mean


ObjMeshTables = abi.struct('vpho_obj_mesh_tables')
ObjMeshAccel = abi.struct('vpho_obj_mesh_accel')
ObjSolids = abi.struct('vpho_obj_solids')
ObjSolidColumns = abi.struct('vpho_obj_solid_columns')


VOLUME_MULTI_MAX_PAIRS = 0x7fffffff      # vpho_hand_obj_intersection_multi_f64: one workgroup per (image, hypothesis) on grid.x


class HandObjectPenetration:
    """Hand-object penetration and contact (--eval_physics) on the device: per-triangle tables of every object mesh,
    built once (physics_eval.mesh_tables), + thin wrapper of vpho_hand_obj_penetration_f64.  ``meshes``: {name: {'verts', 'faces'}}
    (physics_eval.object_meshes).  ``multi`` scores every sampled hypothesis (vpho_hand_obj_penetration_multi_f64) through the
    acceleration tables of physics_eval.mesh_accel, built here once as well (``accel=False`` leaves them out: ``multi`` then raises until
    ``build_accel()`` is called).  ``volume`` is the hand-object intersection volume (--eval_volume, vpho_hand_obj_intersection_f64) of a
    hand mesh (``hand_faces``: one closed (F, 3) face list, physics_eval.hand_faces) with the objects' solid point sets, which
    ``build_solids(pitch)`` makes once per pitch.  ``volume_multi`` is that volume for every sampled hypothesis
    (vpho_hand_obj_intersection_multi_f64), a walk of the solids' lattice columns (``build_solid_columns(pitch)``, once per pitch)."""

    def __init__(self, meshes, device, accel=True, hand_faces=None):
        import numpy as np
        from .physics_eval import mesh_tables
        self.names = list(meshes.keys())
        self.name_to_id = {n: i for i, n in enumerate(self.names)}
        tabs = [mesh_tables(meshes[n]['verts'], meshes[n]['faces']) for n in self.names]
        counts = [t[0].shape[0] for t in tabs]
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)
        self.tri = d(np.concatenate([t[0] for t in tabs]))
        self.tri_offset = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(device)
        self.scale = d(np.stack([t[1] for t in tabs]))
        self.translate = d(np.stack([t[2] for t in tabs]))
        self.n_tri = counts
        self.device = device
        self._tabs, self.acc = tabs, None
        self._meshes, self._solids, self._columns, self.hand_faces = meshes, {}, {}, None
        if hand_faces is not None:
            self.set_hand_faces(hand_faces)
        if accel:
            self.build_accel()
        self.c = ObjMeshTables(self.tri.data_ptr(), self.tri_offset.data_ptr(), self.scale.data_ptr(), self.translate.data_ptr(),
                               len(self.names))

    def build_accel(self):
        """vpho_obj_mesh_accel of all objects, once: per-object tables concatenated, triangle indices made global"""
        import numpy as np
        from .physics_eval import mesh_accel
        if self.acc is not None:
            return
        tabs, counts, device = self._tabs, self.n_tri, self.device
        acc = [mesh_accel(t[0]) for t in tabs]
        tri0 = np.concatenate([[0], np.cumsum(counts)])
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(device)
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)
        ent0 = np.concatenate([[0], np.cumsum([len(a['col_tri']) for a in acc])])
        self.col_offset = i32(np.concatenate([a['col_offset'][:-1].astype(np.int64) + ent0[i] for i, a in enumerate(acc)] + [ent0[-1:]]))
        self.col_tri = i32(np.concatenate([a['col_tri'].astype(np.int64) + tri0[i] for i, a in enumerate(acc)]))
        self.clu_offset = i32(np.concatenate([[0], np.cumsum([len(a['sphere']) for a in acc])]))
        self.clu_sphere = f64(np.concatenate([a['sphere'] for a in acc]))
        self.clu_geo = f64(np.concatenate([a['geo'] for a in acc]))
        self.acc = ObjMeshAccel(self.col_offset.data_ptr(), self.col_tri.data_ptr(), self.clu_offset.data_ptr(), self.clu_sphere.data_ptr(),
                                self.clu_geo.data_ptr())

    def set_hand_faces(self, faces):
        """the closed face list of the hand mesh for ``volume``: (F, 3) integers, kept on the device as int32"""
        import numpy as np
        f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int64)
        if f.shape[0] == 0 or f.min() < 0 or f.max() > 0x7fffffff:
            raise VphoError(f'HandObjectPenetration: a hand mesh of {f.shape[0]} faces (indices {f.min() if f.size else None} .. {f.max() if f.size else None})')
        self.hand_faces = torch.as_tensor(f.astype(np.int32)).to(self.device)
        self.hand_faces_max = int(f.max())

    def build_solids(self, pitch):
        """The objects' solid point sets at one voxel pitch (m), once per pitch: per object the cell centres of
        physics_eval.solid_lattice that the single-pose kernel finds inside the object at identity pose (p = v exactly), concatenated,
        plus offsets.  -> dict(pts (P, 3) fp32 and pt_offset (n_obj + 1,) int32 on the device, counts, dims, max_pts, c = ObjSolids)."""
        import numpy as np
        from .physics_eval import solid_lattice
        key = float(pitch)
        if not key > 0.0:
            raise VphoError(f'HandObjectPenetration.build_solids: the voxel pitch must be positive ({pitch})')
        if key in self._solids:
            return self._solids[key]
        eye = torch.zeros((1, 3, 4), dtype=torch.float64, device=self.device)
        eye[0, :, :3] = torch.eye(3, dtype=torch.float64)
        pts, counts, dims = [], [], []
        for o, n in enumerate(self.names):
            c, d = solid_lattice(self._meshes[n]['verts'], self._meshes[n]['faces'], key)
            c = torch.from_numpy(c).to(self.device)
            _, _, inside = self(c[None], eye, [o], per_vertex=True)
            keep = c[inside[0].bool()]
            pts.append(keep)
            counts.append(int(keep.shape[0]))
            dims.append(tuple(int(x) for x in d))
        allp = torch.cat(pts, 0).contiguous() if sum(counts) else torch.zeros((1, 3), dtype=torch.float32, device=self.device)
        off = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(self.device)
        sol = dict(pts=allp, pt_offset=off, counts=counts, dims=dims, max_pts=max(counts), pitch=key)
        sol['c'] = ObjSolids(allp.data_ptr(), off.data_ptr(), len(self.names), sol['max_pts'])
        torch.cuda.current_stream(allp.device).synchronize()          # built on this stream, read by kernels of any stream afterwards
        self._solids[key] = sol
        return sol

    def volume(self, verts, obj_rt, obj_id, pitch=None, flags=False):
        """Hand-object intersection volume per (hand, object pose) pair: verts (n,V,3) fp32 hand vertices and obj_rt (n,3,4) fp64 object
        poses in the camera frame, obj_id as in __call__; ``pitch`` (m; default cfg.physics_voxel_pitch).  -> (n,2) fp64 = n_cells (solid
        cell centres of the object inside the posed hand mesh) | IV = n_cells * pitch^3 (m^3); with ``flags`` also (n, max_pts) uint8,
        one flag per solid centre of the pair's object in the order of build_solids(pitch) (0 behind its last centre)."""
        pitch = self._check_pitch(pitch, 'volume')
        if self.hand_faces is None:
            raise VphoError('HandObjectPenetration.volume: no hand mesh (pass hand_faces= or call set_hand_faces)')
        n, V = verts.shape[:2]
        assert verts.shape == (n, V, 3) and obj_rt.shape == (n, 3, 4)
        if self.hand_faces_max >= V:
            raise VphoError(f'HandObjectPenetration.volume: the hand faces index vertex {self.hand_faces_max}, the hands have {V}')
        obj_id = self._check_ids(obj_id, n)
        sol = self.build_solids(pitch)
        F_ = int(self.hand_faces.shape[0])
        out = _new((n, 2), obj_rt, torch.float64)
        fl = _new((n, sol['max_pts']), obj_rt, torch.uint8) if flags else None
        if n == 0:
            return (out, fl) if flags else out
        need = abi.query('vpho_hand_obj_intersection_workspace_bytes', n, F_)
        if need < 0:
            raise VphoError('vpho_hand_obj_intersection_workspace_bytes: bad argument')
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)          # per call: one object serves streams that run concurrently
        _call('vpho_hand_obj_intersection_f64', C.byref(self.c), C.byref(sol['c']), self.hand_faces, F_, verts, n, V, obj_rt, obj_id, pitch, out, fl,
              ws, ws.numel())
        return (out, fl) if flags else out

    def build_solid_columns(self, pitch):
        """The lattice columns of the objects' solids at one voxel pitch, once per pitch: physics_eval.solid_columns of every object's
        part of build_solids(pitch)['pts'] (which is built first if need be, and stays as it is), run starts made global and concatenated.
        -> dict(col_start (C + 1,) and col_offset (n_obj + 1,) int32 on the device, counts, max_cols, c = ObjSolidColumns)."""
        import numpy as np
        from .physics_eval import solid_columns
        sol = self.build_solids(pitch)
        key = sol['pitch']
        if key in self._columns:
            return self._columns[key]
        pts = sol['pts'].cpu().numpy()
        off = np.concatenate([[0], np.cumsum(sol['counts'])]).astype(np.int64)
        starts, counts = [], []
        for o in range(len(self.names)):
            cs = solid_columns(pts[off[o]:off[o + 1]])
            starts.append(cs[:-1].astype(np.int64) + off[o])
            counts.append(len(cs) - 1)
        col_start = torch.as_tensor(np.concatenate(starts + [off[-1:]]).astype(np.int32)).to(self.device)
        col_offset = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(self.device)
        cols = dict(col_start=col_start, col_offset=col_offset, counts=counts, max_cols=max(counts), pitch=key)
        cols['c'] = ObjSolidColumns(col_start.data_ptr(), col_offset.data_ptr(), len(self.names), cols['max_cols'])
        torch.cuda.current_stream(col_start.device).synchronize()     # built on this stream, read by kernels of any stream afterwards
        self._columns[key] = cols
        return cols

    def volume_multi(self, verts, obj_rt, obj_id, pitch=None, flags=False):
        """The intersection volume of every sampled hypothesis: verts (n,S,V,3) fp32 and obj_rt (n,S,3,4) fp64 in the camera frame,
        hypothesis s of the hand against hypothesis s of the object; obj_id as in __call__ (one per image); ``pitch`` as in ``volume``.
        -> table (n,6) fp64 in the order of ops_names.VOLUME_MULTI_COLUMNS (hypothesis 0 | the minima over S | mean_cells = integer sum /
        S and mean_IV = pitch^3 * mean_cells; a NaN hypothesis makes best and mean NaN) and per_hyp (n,S,2) fp64 = n_cells | IV, the bits
        ``volume`` gives for the n*S pairs; with ``flags`` also (n,S,max_pts) uint8 with its bits.  n * S <= VOLUME_MULTI_MAX_PAIRS."""
        pitch = self._check_pitch(pitch, 'volume_multi')
        if self.hand_faces is None:
            raise VphoError('HandObjectPenetration.volume_multi: no hand mesh (pass hand_faces= or call set_hand_faces)')
        n, S, V = verts.shape[:3]
        assert verts.shape == (n, S, V, 3) and obj_rt.shape == (n, S, 3, 4)
        if S < 1:
            raise VphoError(f'HandObjectPenetration.volume_multi: no hypotheses (S={S})')
        if n * S > VOLUME_MULTI_MAX_PAIRS:
            raise VphoError(f'HandObjectPenetration.volume_multi: {n} x {S} pairs, at most {VOLUME_MULTI_MAX_PAIRS} in one call')
        if self.hand_faces_max >= V:
            raise VphoError(f'HandObjectPenetration.volume_multi: the hand faces index vertex {self.hand_faces_max}, the hands have {V}')
        obj_id = self._check_ids(obj_id, n)
        sol = self.build_solids(pitch)
        cols = self.build_solid_columns(pitch)
        F_ = int(self.hand_faces.shape[0])
        table = _new((n, 6), obj_rt, torch.float64)
        per = _new((n, S, 2), obj_rt, torch.float64)
        fl = _new((n, S, sol['max_pts']), obj_rt, torch.uint8) if flags else None
        if n == 0:
            return (table, per, fl) if flags else (table, per)
        need = abi.query('vpho_hand_obj_intersection_multi_workspace_bytes', n, S, F_)
        if need < 0:
            raise VphoError('vpho_hand_obj_intersection_multi_workspace_bytes: bad argument')
        ws = torch.empty(need, dtype=torch.uint8, device=self.device) if need else None       # per call, as in volume
        _call('vpho_hand_obj_intersection_multi_f64', C.byref(self.c), C.byref(sol['c']), C.byref(cols['c']), self.hand_faces, F_, verts, n, S, V,
              obj_rt, obj_id, pitch, per, table, fl, ws, need)
        return (table, per, fl) if flags else (table, per)

    def _check_ids(self, obj_id, n):
        """obj_id of the four metric calls as an (n,) device tensor: a host sequence of ints is range-checked and copied"""
        if not torch.is_tensor(obj_id):
            ids = [int(i) for i in obj_id]
            if len(ids) != n or any(i < 0 or i >= len(self.names) for i in ids):
                raise VphoError(f'HandObjectPenetration: object ids {ids} outside [0, {len(self.names)}) or not one per image')
            obj_id = _ids_to_device(ids, self.device)
        assert obj_id.shape == (n,)
        return obj_id

    @staticmethod
    def _check_pitch(pitch, who):
        """the voxel pitch (m) of ``volume`` / ``volume_multi`` as a float; default cfg.physics_voxel_pitch"""
        if pitch is None:
            from .configs.args import cfg
            pitch = cfg.physics_voxel_pitch
        pitch = float(pitch)
        if not pitch > 0.0:
            raise VphoError(f'HandObjectPenetration.{who}: the voxel pitch must be positive ({pitch})')
        return pitch

    def obj_ids(self, names):
        """class indices of a batch as a device tensor (pinned host memory, asynchronous copy on the caller's stream, as
        ObjectMetrics.obj_ids); an unknown name raises VphoError"""
        bad = [n for n in names if n not in self.name_to_id]
        if bad:
            raise VphoError(f'HandObjectPenetration: no mesh for the objects {bad}')
        return _ids_to_device([self.name_to_id[n] for n in names], self.device)

    def __call__(self, verts, obj_rt, obj_id, contact_thresh=0.005, per_vertex=False):
        """verts (n,V,3) fp32 hand vertices and obj_rt (n,3,4) fp64 [R | t] object poses, both in the camera frame; obj_id: (n,) int32
        device tensor (obj_ids) or a host sequence of ints, which is range-checked here (the kernel cannot refuse a device id without
        a host sync: an out-of-range device id gives NaN rows).  -> per_image (n,4) fp64 = PD (m), n_inside, min sd (m), contact;
        with per_vertex also sd (n,V) fp64 and inside (n,V) uint8."""
        n, V = verts.shape[:2]
        assert verts.shape == (n, V, 3) and obj_rt.shape == (n, 3, 4)
        obj_id = self._check_ids(obj_id, n)
        per = _new((n, 4), obj_rt, torch.float64)
        sd = _new((n, V), obj_rt, torch.float64)
        inside = _new((n, V), obj_rt, torch.uint8)
        _call('vpho_hand_obj_penetration_f64', C.byref(self.c), verts, n, V, obj_rt, obj_id, contact_thresh, sd, inside, per)
        return (per, sd, inside) if per_vertex else per

    def multi(self, verts, obj_rt, obj_id, per_vertex=False, contact_thresh=0.005):
        """Every sampled hypothesis: verts (n,S,V,3) fp32 and obj_rt (n,S,3,4) fp64 in the camera frame, hypothesis s of the hand against
        hypothesis s of the object; obj_id as in __call__ (one per image).  -> table (n,12) fp64 = one | best | mean over S of
        (PD, n_inside, min sd, contact): hypothesis 0; min PD, min n_inside, max min-sd, max contact; the four means -- and per_hyp
        (n,S,4) fp64, the bits __call__ gives for the n*S pairs.  With per_vertex also sd (n,S,V) fp64 and inside (n,S,V) uint8;
        without it nothing is written per vertex."""
        if self.acc is None:
            raise VphoError('HandObjectPenetration.multi: built with accel=False (call build_accel() first)')
        n, S, V = verts.shape[:3]
        assert verts.shape == (n, S, V, 3) and obj_rt.shape == (n, S, 3, 4)
        obj_id = self._check_ids(obj_id, n)
        table = _new((n, 12), obj_rt, torch.float64)
        per = _new((n, S, 4), obj_rt, torch.float64)
        sd = _new((n, S, V), obj_rt, torch.float64) if per_vertex else None
        inside = _new((n, S, V), obj_rt, torch.uint8) if per_vertex else None
        _call('vpho_hand_obj_penetration_multi_f64', C.byref(self.c), C.byref(self.acc), verts, n, S, V, obj_rt, obj_id, contact_thresh, per,
              sd if per_vertex else None, inside if per_vertex else None, table)
        return (table, per, sd, inside) if per_vertex else (table, per)


ObjVertexAccel = abi.struct('vpho_obj_vertex_accel')


class ContactMulti:
    """The hand contact map of every sampled hypothesis (--eval_grasp; csrc/contact_multi.hip): the hand -> object
    half of detect_hand_and_object_contact for n x S pairs in the object's model frame.  ``tables``: the host arrays of
    grasp_eval.vertex_accel_tables (vpho_obj_vertex_accel of all objects, in the order of the object ids), kept on the device here."""

    def __init__(self, tables, device):
        import numpy as np
        if not torch.device(device).type == 'cuda':
            raise VphoError('vpho_amd ops take GPU tensors only (no CPU path)')
        dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(device)
        self.vert, self.sphere = dev(tables['vert'], np.float64), dev(tables['clu_sphere'], np.float64)
        self.index, self.clu_offset, self.clu_start = (dev(tables[k], np.int32) for k in ('index', 'clu_offset', 'clu_start'))
        self.n_obj, self.device = len(tables['clu_offset']) - 1, device
        if self.n_obj < 1 or self.vert.shape[0] < 1 or self.vert.shape != (self.index.shape[0], 3) or self.sphere.shape != (self.clu_start.shape[0] - 1, 4):
            raise VphoError(f'ContactMulti: tables of {self.n_obj} objects, vert {tuple(self.vert.shape)}, index {tuple(self.index.shape)}, '
                            f'clu_sphere {tuple(self.sphere.shape)}, clu_start {tuple(self.clu_start.shape)}')
        self.c = ObjVertexAccel(self.vert.data_ptr(), self.index.data_ptr(), self.clu_offset.data_ptr(), self.clu_start.data_ptr(),
                                self.sphere.data_ptr(), self.n_obj)

    def __call__(self, hand_verts, hand_normals, root, is_right, obj_rt, obj_id, normal_thresh=(-0.015, 0.01), vertical_thresh=0.01,
                 decay=(-0.005, 0.005), per_vertex=False):
        """hand_verts, hand_normals (n,S,Nh,3) fp32: the filled surface of HandSurface.fill in its flipped, root-relative frame; root (n,3)
        fp64, is_right (n,) uint8, obj_rt (n,S,3,4) fp64 in the camera frame, obj_id (n,) int32 device tensor (an id outside the table
        gives NaN rows: it cannot be refused without a host sync).  -> weight (n,S,Nh) fp32 in [0, 1]; with per_vertex also nn_index
        (n,S,Nh) int32 (-1 without contact) and nd, vd (n,S,Nh) fp64."""
        n, S, Nh = hand_verts.shape[:3]
        if hand_verts.shape != (n, S, Nh, 3) or hand_normals.shape != hand_verts.shape or obj_rt.shape != (n, S, 3, 4) or root.shape != (n, 3) \
                or is_right.shape != (n,) or obj_id.shape != (n,):
            raise VphoError(f'ContactMulti: hand_verts {tuple(hand_verts.shape)}, hand_normals {tuple(hand_normals.shape)}, root {tuple(root.shape)}, '
                            f'is_right {tuple(is_right.shape)}, obj_rt {tuple(obj_rt.shape)}, obj_id {tuple(obj_id.shape)}')
        w = _new((n, S, Nh), hand_verts)
        nn = _new((n, S, Nh), hand_verts, torch.int32) if per_vertex else None
        nd, vd = (_new((n, S, Nh), hand_verts, torch.float64) for _ in range(2)) if per_vertex else (None, None)
        _call('vpho_contact_multi_f32', C.byref(self.c), hand_verts, hand_normals, n, S, Nh, root, is_right, obj_rt, obj_id, normal_thresh[0],
              normal_thresh[1], vertical_thresh, decay[0], decay[1], w, nn, nd, vd)
        return (w, nn, nd, vd) if per_vertex else w


def contact_agreement(weight, weight_gt, force_contact, is_grasped, force_contact_gt, is_grasped_gt):
    """vpho_contact_agreement_f32: weight (n,S,Nh) against weight_gt (n,Nh) fp32, force_contact (n,S,32) fp32 / is_grasped (n,S) uint8
    against their (n,32) / (n,) counterparts -> counts (n,S,3) int32 = TP, P, G; values (n,S,8) fp64 in the order of
    ops_names.GRASP_METRIC_NAMES; table (n,24) fp64 = hypothesis 0 | best-of-S | mean-of-S"""
    n, S, Nh = weight.shape
    if weight_gt.shape != (n, Nh) or force_contact.shape != (n, S, 32) or is_grasped.shape != (n, S) or force_contact_gt.shape != (n, 32) \
            or is_grasped_gt.shape != (n,):
        raise VphoError(f'contact_agreement: weight {tuple(weight.shape)}, weight_gt {tuple(weight_gt.shape)}, force_contact {tuple(force_contact.shape)}, '
                        f'is_grasped {tuple(is_grasped.shape)}, force_contact_gt {tuple(force_contact_gt.shape)}, is_grasped_gt {tuple(is_grasped_gt.shape)}')
    counts = _new((n, S, 3), weight, torch.int32)
    values, table = _new((n, S, 8), weight, torch.float64), _new((n, 24), weight, torch.float64)
    _call('vpho_contact_agreement_f32', weight, weight_gt, force_contact, is_grasped, force_contact_gt, is_grasped_gt, n, S, Nh, counts, values,
          table)
    return counts, values, table


# ----------------------------------------------------------------------------------------------- score-network training
def linear_into(x, w, bias, out, c_off, out_slope=1.0):
    """out[:, c_off : c_off + cout] = act(x @ w.T + bias) for a wider row-major `out` (concatenation buffers)."""
    rows, cin = x.shape
    ld = out.shape[1]
    conv2d_nhwc(x.view(rows, 1, 1, cin), w, bias, out_slope=out_slope, out_view=(out, ld, ld, ld, c_off))
    return out


def dsm_prepare(gt_pose, t, z, fourier_W, Dp):
    """t (reps,bs), z (reps,bs,D) -> x_t (rows,Dp), emb (rows,128), std (rows,)   rows = reps*bs, row = rep*bs + b"""
    reps, bs = t.shape
    D = gt_pose.shape[1]
    xt, emb, sd = _new((reps * bs, Dp), gt_pose), _new((reps * bs, 128), gt_pose), _new((reps * bs,), gt_pose)
    _call('vpho_dsm_prepare_f32', gt_pose, t, z, fourier_W, bs, reps, D, Dp, xt, emb, sd)
    return xt, emb, sd


def plinear2_fwd(h, w2, b2, std_rows, nheads):
    rows = h.shape[0]
    score = _new((rows, 3 * nheads), h)
    _call('vpho_plinear2_fwd_f32', h, w2, b2, std_rows, rows, nheads, score)
    return score


def dsm_loss(score, z, std_rows, batch_times_reps):
    """-> loss (0-d fp64 device tensor), dout (rows,D)"""
    rows, D = score.shape
    dout = torch.empty_like(score)
    loss = _new((), score, torch.float64)
    ws = _new((1024,), score, torch.float64)
    _call('vpho_dsm_loss_f32', score, z, std_rows, rows, D, batch_times_reps, dout, loss, ws, 1024)
    return loss, dout


def mse_loss(pd, gt, weight=1.0):
    """-> weight * mean((pd-gt)^2) (0-d fp64 device tensor), its gradient w.r.t. pd"""
    assert pd.shape == gt.shape
    grad = torch.empty_like(pd)
    loss = _new((), pd, torch.float64)
    ws = _new((1024,), pd, torch.float64)
    _call('vpho_mse_loss_f32', pd, gt, pd.numel(), weight, grad, loss, ws, 1024)
    return loss, grad


def plinear2_bwd(h, dout, w2, nheads):
    rows = h.shape[0]
    dpre, dw2, db2 = torch.empty_like(h), torch.empty_like(w2), _new((nheads, 3), h)
    _call('vpho_plinear2_bwd_f32', h, dout, w2, rows, nheads, dpre, dw2, db2)
    return dpre, dw2, db2


def relu_bwd(dy, dy_off, ld_dy, y, y_off, ld_y, rows, cols):
    """contiguous (rows, cols) = where(y_slice > 0, dy_slice, 0); slices are given by element offset + leading dimension"""
    dx = _new((rows, cols), dy)
    _call('vpho_relu_bwd_f32', abi.at(dy, torch.float32, dy_off), ld_dy, abi.at(y, torch.float32, y_off), ld_y, rows, cols, dx, cols)
    return dx


def colsum(x):
    rows, cols = x.shape
    out = _new((cols,), x)
    ws = _bn_workspace(cols, x.device)
    _call('vpho_colsum_f32', x, cols, rows, cols, out, ws)
    return out


def sum_repeats(x, c_off, bs, reps, cols):
    out = _new((bs, cols), x)
    _call('vpho_sum_repeats_f32', x, x.shape[1], c_off, bs, reps, cols, out)
    return out


def transpose(x, pad_to=4):
    """(rows, cols) -> (cols, rows rounded up to a multiple of pad_to), the padding columns zero (GEMM operands want a
    reduction length that is a multiple of 4)"""
    rows, cols = x.shape
    rp = (rows + pad_to - 1) // pad_to * pad_to
    y = _new((cols, rp), x) if rp == rows else torch.zeros((cols, rp), device=x.device, dtype=x.dtype)
    _call('vpho_transpose_f32', x, rows, cols, cols, y, rp)
    return y


def im2col_t(x, kh, kw, stride, pad_y, pad_x, OH, OW, cin=None):
    """x (N,H,W,ld) NHWC -> (kh*kw*cin, P rounded up to a multiple of 4) with P = N*OH*OW; see vpho_im2col_t_f32"""
    N, H, W, ld = x.shape
    cin = ld if cin is None else cin
    P = N * OH * OW
    ldo = (P + 3) // 4 * 4
    out = _new((kh * kw * cin, ldo), x)
    _call('vpho_im2col_t_f32', x, N, H, W, cin, ld, kh, kw, stride, pad_y, pad_x, OH, OW, out, ldo)
    return out


def window_groups(win):
    """live 32-pixel groups of the (N,H,W) map of a ``RoiWindows`` (ascending list + count, device tensors): where a gradient that
    came back through RoIAlign can be non-zero (vpho_window_groups_i32)"""
    N, H, W = win.shape
    lst = torch.empty((N * H * W // 32,), device=win.wins.device, dtype=torch.int32)
    cnt = torch.empty((1,), device=win.wins.device, dtype=torch.int32)
    _call('vpho_window_groups_i32', win.wins, N, H, W, lst, cnt)
    return lst, cnt


def conv2d_wgrad_nhwc(x, dy, kh, kw, stride, pad_y, pad_x, cin=None, groups=None):
    """x (N,H,W,ld), dy (N,OH,OW,Cout) contiguous -> dW (Cout, kh*kw*cin) packed; implicit TN GEMM (csrc/conv_wgrad.hip).
    ``groups`` = window_groups(...) of the OUTPUT map: dy is zero outside them, the reduction skips everything else."""
    N, H, W, ld = x.shape
    _, OH, OW, cout = dy.shape
    cin = ld if cin is None else cin
    dw = _new((cout, kh * kw * cin), x)
    nbytes = abi.query('vpho_conv2d_wgrad_workspace_bytes', N, OH, OW, cin, cout, kh, kw)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes > 0 else None
    if groups is not None and OW % 32 == 0:
        _call('vpho_conv2d_wgrad_groups_nhwc_f32', x, N, H, W, cin, ld, dy, OH, OW, cout, cout, kh, kw, stride, pad_y, pad_x, groups[0], groups[1],
              dw, ws)
        return dw
    _call('vpho_conv2d_wgrad_nhwc_f32', x, N, H, W, cin, ld, dy, OH, OW, cout, cout, kh, kw, stride, pad_y, pad_x, dw, ws)
    return dw


_BN_WS = {}


def _bn_workspace(Cc, device):
    """scratch of the BatchNorm reductions (256 chunks x 2 x C doubles), one per (device, stream): every user is stream-ordered and done with it
    when its call's last kernel has run; allocating it per call cost the training step ~270 allocator round trips"""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    need = abi.query('vpho_bn_workspace_bytes', Cc)
    ws = _BN_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _BN_WS[key] = torch.empty(max(need, 256 * 2 * 2048 * 8), dtype=torch.uint8, device=device)
    return ws


def bn_train_forward(x, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1, slope=1.0, res=None, partials=None):
    """x (..., C) NHWC -> y, (save_mean, save_invstd); running stats updated in place (nn.BatchNorm2d.train()).
    partials: the BnFuse the convolution that produced x filled -- the reduction pass over x is then skipped"""
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y, mean, invstd = torch.empty_like(x), _new((Cc,), x), _new((Cc,), x)
    ws = _bn_workspace(Cc, x.device)
    if partials is not None and partials.live():
        assert partials.stats.shape[-1] == Cc
        _call('vpho_bn_train_forward_stats_f32', x, rows, Cc, Cc, partials.stats, partials.rows, gamma, beta, eps, momentum, slope, running_mean,
              running_var, mean, invstd, res, y, ws)
        return y, (mean, invstd)
    _call('vpho_bn_train_forward_f32', x, rows, Cc, Cc, gamma, beta, eps, momentum, slope, running_mean, running_var, mean, invstd, res, y, ws)
    return y, (mean, invstd)


def bn_train_backward(x, dy, gamma, saved, partials=None, res=None, want_colsum=False):
    """-> dx, dgamma, dbeta (, column sums of dx).  partials: the BnFuse the convolution that produced dy filled (sum dy | sum dy * xhat).
    res: a gradient of x's shape added to dx (the identity shortcut of a pre-activation residual block); want_colsum: also return the
    column sums of the stored dx (the bias gradient of the convolution that produced x), taken while dx is written"""
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    dx, dg, db = torch.empty_like(x), _new((Cc,), x), _new((Cc,), x)
    ws = _bn_workspace(Cc, x.device)
    live = partials is not None and partials.x is not None and partials.live()
    if live or res is not None or want_colsum:
        cs = _new((Cc,), x) if want_colsum else None
        if live:
            assert partials.stats.shape[-1] == Cc
        assert res is None or (res.shape == x.shape and res.is_contiguous())
        _call('vpho_bn_train_backward_stats_f32', x, dy, rows, Cc, Cc, gamma, saved[0], saved[1], partials.stats if live else None,
              partials.rows if live else 0, res, dx, dg, db, cs, ws)
        return (dx, dg, db, cs) if want_colsum else (dx, dg, db)
    _call('vpho_bn_train_backward_f32', x, dy, rows, Cc, Cc, gamma, saved[0], saved[1], dx, dg, db, ws)
    return dx, dg, db


def lrelu_bwd(dy, y, slope):
    dx = torch.empty_like(dy)
    _call('vpho_lrelu_bwd_f32', dy, y, dy.numel(), slope, dx)
    return dx


def maxpool_bwd(x, dy, k, stride, pad, one_pass=False):
    """one_pass: the gather that scans every window itself (vpho_maxpool_bwd_nhwc_f32), also where the windows overlap"""
    N, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    if one_pass:
        _call('vpho_maxpool_bwd_nhwc_f32', x, dy, N, H, W, Cc, k, stride, pad, dx)
        return dx
    need = abi.query('vpho_maxpool_bwd_workspace_bytes', N, H, W, Cc, k, stride, pad)
    ws = torch.empty(need, dtype=torch.uint8, device=x.device) if need > 0 else None
    _call('vpho_maxpool_bwd_ws_nhwc_f32', x, dy, N, H, W, Cc, k, stride, pad, dx, abi.at(ws, torch.uint8))
    return dx


def resize_bilinear_bwd(dy, H, W):
    N, OH, OW, Cc = dy.shape
    dx = _new((N, H, W, Cc), dy)
    _call('vpho_resize_bilinear_bwd_nhwc_f32', dy, N, OH, OW, Cc, H, W, dx)
    return dx


def roi_align_bwd(dy, boxes, feat_hw, C, scale, flip_w=None, c_off=0, into=None):
    """dy (N,P,P,ld) -> feature gradient (N,H,W,C); `into` accumulates into an existing gradient tensor"""
    N, P, _, ld = dy.shape
    H, W = feat_hw
    df = torch.zeros((N, H, W, C), device=dy.device, dtype=dy.dtype) if into is None else into
    _call('vpho_roi_align_bwd_nhwc_f32', dy, ld, c_off, N, H, W, C, boxes, scale, P, flip_w, df)
    return df


def align_heatmap_bwd(dout, bbox, bbox_rect, flip_w=None):
    N, S, _, Cc = dout.shape
    dhm = torch.zeros_like(dout)
    _call('vpho_align_heatmap_bwd_nhwc_f32', dout, N, S, Cc, bbox, bbox_rect, flip_w, dhm)
    return dhm


def add_lrelu(a, b, slope=1.0):
    y = torch.empty_like(a)
    _call('vpho_add_lrelu_f32', a, b, a.numel(), slope, y)
    return y


def adamw_(param, grad, m, v, step, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0):
    """in-place torch.optim.AdamW step on one tensor"""
    _call('vpho_adamw_f32', param, grad, m, v, param.numel(), lr, beta1, beta2, eps, weight_decay, step, grad_scale)


class AdamWList:
    """torch.optim.AdamW on a fixed list of (param, grad, exp_avg, exp_avg_sq) tensors as ONE launch (vpho_adamw_multi_f32)"""
    def __init__(self, quads):
        self.keep = quads
        rows, blk = [], 0
        for p, g, m, v in quads:
            for t in (p, g, m, v):
                _f32p(t)
            assert p.numel() == g.numel() == m.numel() == v.numel()
            rows.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), blk])
            blk += (p.numel() + 1023) // 1024
        self.blocks, self.n = blk, len(rows)
        self.table = torch.tensor(rows, dtype=torch.int64).to(quads[0][0].device)

    def step(self, step, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0):
        _call('vpho_adamw_multi_f32', abi.at(self.table, torch.int64), self.n, self.blocks, lr, beta1, beta2, eps, weight_decay, step, grad_scale)
        # the kernel wrote through raw pointers: tell torch, so that everything cached per weight VERSION (the Winograd transforms of
        # winograd_weights_device, the bf16 planes) is rebuilt -- no launch, a counter per tensor
        torch.autograd.graph.increment_version([q[0] for q in self.keep])


def grad_sqnorm(flat, ws=None, out=None):
    """sum of squares of a contiguous fp32 buffer -> 0-d fp64 tensor that stays on the device (fixed summation order: two runs give the
    same bits).  ``ws``: a uint8 workspace of at least ``grad_sqnorm_workspace_bytes(n)`` bytes to reuse; ``out``: a 0-d fp64 tensor to write"""
    n = flat.numel()
    need = abi.query('vpho_grad_sqnorm_workspace_bytes', n)
    if need < 0:
        raise VphoError(f'vpho_grad_sqnorm_workspace_bytes: bad argument (n={n})')
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.float64, device=flat.device)
    elif ws.numel() * ws.element_size() < need:
        raise VphoError(f'grad_sqnorm: a workspace of {ws.numel() * ws.element_size()} bytes, {need} are needed')
    if out is None:
        out = _new((), flat, torch.float64)
    _call('vpho_grad_sqnorm_f64', flat, n, out, ws)
    return out


def grad_sqnorm_workspace_bytes(n):
    return int(abi.query('vpho_grad_sqnorm_workspace_bytes', n))


OPTIM_KINDS = {'adamw': 0, 'adam': 1}


class OptimList:
    """torch.optim.AdamW (kind 0) or torch.optim.Adam with L2 decay (kind 1) on a fixed list of (param, grad, exp_avg, exp_avg_sq) tensors
    as ONE launch (vpho_optim_multi_f32).  ``sqnorm`` (0-d fp64 device tensor from ``grad_sqnorm`` of the summed gradients) + ``max_norm``:
    the kernel forms clip_grad_norm_'s coefficient itself; the gradients are never written."""
    def __init__(self, quads):
        self.keep = quads
        rows, blk = [], 0
        for p, g, m, v in quads:
            for t in (p, g, m, v):
                _f32p(t)
            assert p.numel() == g.numel() == m.numel() == v.numel()
            rows.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), blk])
            blk += (p.numel() + 1023) // 1024
        self.blocks, self.n = blk, len(rows)
        self.table = torch.tensor(rows, dtype=torch.int64).to(quads[0][0].device)

    def step(self, step, kind=0, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0, sqnorm=None, max_norm=0.0):
        if sqnorm is not None and not (sqnorm.numel() == 1 and max_norm > 0):
            raise VphoError(f'OptimList.step: clipping needs one fp64 value and max_norm > 0 (got {tuple(sqnorm.shape)}, {max_norm})')
        _call('vpho_optim_multi_f32', abi.at(self.table, torch.int64), self.n, self.blocks, OPTIM_KINDS.get(kind, kind), lr, beta1, beta2, eps, weight_decay, step,
              grad_scale, sqnorm, max_norm)
        # raw-pointer writes: bump the version counters, as AdamWList.step does (Winograd transforms and bf16 planes are cached per version)
        torch.autograd.graph.increment_version([q[0] for q in self.keep])


class EmaList:
    """ExponentialMovingAverage.update (lib/model/ema.py:25-44) on a fixed list of (param, shadow) fp32 tensors as ONE launch
    (vpho_ema_multi_f32): shadow -= one_minus_decay * (shadow - param), the three fp32 roundings of torch's own expression.  The
    parameters are only read.  An empty list launches nothing."""
    def __init__(self, pairs):
        self.keep = pairs
        rows, blk = [], 0
        for p, s in pairs:
            for t in (p, s):
                _f32p(t)
            if p.device != s.device:
                raise VphoError(f'EmaList: parameter on {p.device}, shadow on {s.device}')
            if p.numel() != s.numel():
                raise VphoError(f'EmaList: a parameter of {p.numel()} elements with a shadow of {s.numel()}')
            rows.append([p.data_ptr(), s.data_ptr(), p.numel(), blk])
            blk += (p.numel() + 1023) // 1024
        self.blocks, self.n = blk, len(rows)
        self.table = torch.tensor(rows, dtype=torch.int64).to(pairs[0][0].device) if rows else None

    def update(self, one_minus_decay):
        if self.n == 0:
            return
        _call('vpho_ema_multi_f32', abi.at(self.table, torch.int64), self.n, self.blocks, one_minus_decay)
        torch.autograd.graph.increment_version([q[1] for q in self.keep])


# ----------------------------------------------------------------------------------------------- frames in (frames.hip)
def frame_patch(frames, minv, patch, colour=None, flip=None, erase=None, key=None, out=None):
    """(n,H,W,3) uint8 frames -> (n,3,patch,patch) fp32 normalised crops (vpho_frame_patch_f32: dexycb6.py:345,389-399,442-444).
    ``minv`` (n,6) fp64: rows 0-1 of the inverse crop matrix (patch -> frame).  Optional, per sample: ``colour`` (n,5) fp32 dr, dg, db,
    brightness, saturation; ``flip`` (n) uint8; ``erase`` (n,4,4) int32 rectangles x0, y0, x1, y1 in output coordinates with ``key``
    (n,2) int32 holding the two uint32 words of the Philox key.  n == 0 launches nothing."""
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise VphoError(f'frame_patch: frames of shape {tuple(frames.shape)}, expected (n, H, W, 3)')
    n, H, W, _ = frames.shape
    for name, t, shape in (('minv', minv, (n, 6)), ('colour', colour, (n, 5)), ('flip', flip, (n,)), ('erase', erase, (n, 4, 4)), ('key', key, (n, 2))):
        if t is not None and tuple(t.shape) != shape:
            raise VphoError(f'frame_patch: {name} of shape {tuple(t.shape)}, expected {shape}')
    if erase is not None and key is None:
        raise VphoError('frame_patch: erase rectangles need a Philox key')
    if out is None:
        out = _new((n, 3, patch, patch), frames)
    elif tuple(out.shape) != (n, 3, patch, patch):
        raise VphoError(f'frame_patch: out of shape {tuple(out.shape)}, expected {(n, 3, patch, patch)}')
    _call('vpho_frame_patch_f32', frames, n, H, W, minv, colour, flip, erase, key, patch, out)
    return out


def heatmap_targets(pts, box, g, sigma, gmin, size, res=None, left=None, out=None):
    """(n,J,2) fp64 patch points -> (n,J,size,size) fp32 heat-map targets (vpho_heatmap_targets_f32, misc_fn.py:285-385).  ``g`` (G,G) fp32
    Gaussian table, ``gmin`` its fp64 minimum.  ``res`` None: HeatmapGenerator.get_heatmap with ``box`` (n,4) fp64 = x0, y0, max_wh, unused
    and ``left`` (n) uint8; ``res`` (n,2) int32: AdaptiveHeatmapGenerator.__call__ with ``box`` = x0, y0, w, h.  n == 0 launches nothing."""
    if pts.dim() != 3 or pts.shape[2] != 2:
        raise VphoError(f'heatmap_targets: points of shape {tuple(pts.shape)}, expected (n, J, 2)')
    n, J, _ = pts.shape
    for name, t, shape in (('box', box, (n, 4)), ('res', res, (n, 2)), ('left', left, (n,))):
        if t is not None and tuple(t.shape) != shape:
            raise VphoError(f'heatmap_targets: {name} of shape {tuple(t.shape)}, expected {shape}')
    if g.dim() != 2 or g.shape[0] != g.shape[1]:
        raise VphoError(f'heatmap_targets: a Gaussian table of shape {tuple(g.shape)}')
    if out is None:
        out = _new((n, J, size, size), pts)
    elif tuple(out.shape) != (n, J, size, size):
        raise VphoError(f'heatmap_targets: out of shape {tuple(out.shape)}, expected {(n, J, size, size)}')
    _call('vpho_heatmap_targets_f32', pts, box, res, left, g, g.shape[0], sigma, gmin, n, J, size, 0 if res is None else 1, out)
    return out


# ----------------------------------------------------------------------------------------------- photometric augmentation (photo.hip)
def _photo_levels(name, levels, clahe=False):
    """the refusals every photo_* op shares, before any launch: (n, P, P, 3) uint8 on the device -> n, P"""
    if not torch.is_tensor(levels) or levels.dim() != 4 or levels.shape[3] != 3 or levels.shape[1] != levels.shape[2] or levels.dtype != torch.uint8:
        raise VphoError(f'{name}: levels must be a (n, P, P, 3) uint8 tensor, got {tuple(levels.shape) if torch.is_tensor(levels) else type(levels)}')
    n, P = int(levels.shape[0]), int(levels.shape[1])
    if n > 65535 or P < 1 or P > 16384:
        raise VphoError(f'{name}: n {n} / P {P} beyond 65535 images of 16384 pixels a side')
    if clahe and P % 8:
        raise VphoError(f'{name}: the 8 x 8 tile grid of CLAHE needs a patch size that is a multiple of 8, got {P}')
    return n, P


def _photo_host_ints(name, what, v, n, ok, rule):
    """a per-sample host parameter (sequence of n integers) checked here, then uploaded as int32"""
    import numpy as np
    a = np.asarray(v.cpu() if torch.is_tensor(v) else v)
    if a.shape != (n,) or a.dtype.kind not in 'iu' or not all(ok(int(k)) for k in a):
        raise VphoError(f'{name}: {what} must be {n} integers, each {rule}; got {a.tolist() if a.size <= 16 else a.shape}')
    return torch.from_numpy(a.astype(np.int32))


def _photo_out(name, out, shape, like, dtype):
    if out is None:
        return _new(shape, like, dtype)
    if tuple(out.shape) != shape or out.dtype != dtype:
        raise VphoError(f'{name}: out of shape {tuple(out.shape)} and dtype {out.dtype}, expected {shape} {dtype}')
    return out


def photo_levels(frames, minv, patch, out=None):
    """(n,H,W,3) uint8 frames -> levels (n,patch,patch,3) uint8: the bicubic crop of ``frame_patch`` before any colour stage, not
    mirrored (vpho_photo_levels_u8)."""
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise VphoError(f'photo_levels: frames of shape {tuple(frames.shape)}, expected (n, H, W, 3)')
    n, H, W, _ = frames.shape
    if tuple(minv.shape) != (n, 6):
        raise VphoError(f'photo_levels: minv of shape {tuple(minv.shape)}, expected {(n, 6)}')
    patch = int(patch)
    if n > 65535 or patch < 1 or patch > 16384:
        raise VphoError(f'photo_levels: n {n} / patch {patch} beyond 65535 images of 16384 pixels a side')
    out = _photo_out('photo_levels', out, (n, patch, patch, 3), frames, torch.uint8)
    _call('vpho_photo_levels_u8', frames, n, H, W, minv, patch, out)
    return out


def photo_clahe_lut(levels, clip):
    """levels -> (l8 (n,P,P) uint8, lut (n,64,256) uint8) of vpho_photo_clahe_lut_u8.  ``clip``: n host integers, the clip COUNT of each
    sample (``photo.clahe_clip``), 0 = the sample's gate is off and its rows of l8 / lut are left unwritten.  Returns clip on the device
    as the third item."""
    n, P = _photo_levels('photo_clahe_lut', levels, clahe=True)
    clip = _photo_host_ints('photo_clahe_lut', 'clip', clip, n, lambda k: 0 <= k <= P * P, 'a clip count in 0 .. P * P').to(levels.device)
    l8, lut = _new((n, P, P), levels, torch.uint8), _new((n, 64, 256), levels, torch.uint8)
    _call('vpho_photo_clahe_lut_u8', levels, clip, n, P, l8, lut)
    return l8, lut, clip


def photo_clahe_apply(levels, clip, l8, lut, out=None, want_l8=False):
    """the interpolation between the tiles' LUTs and the return trip through Lab (vpho_photo_clahe_apply_u8): -> levels, or (levels, l8')
    with ``want_l8``.  ``clip`` (n) int32 on the device, as ``photo_clahe_lut`` returned it.  ``out`` may be ``levels``."""
    n, P = _photo_levels('photo_clahe_apply', levels, clahe=True)
    for name, t, shape, dt in (('clip', clip, (n,), torch.int32), ('l8', l8, (n, P, P), torch.uint8), ('lut', lut, (n, 64, 256), torch.uint8)):
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt:
            raise VphoError(f'photo_clahe_apply: {name} must be {shape} {dt}')
    out = _photo_out('photo_clahe_apply', out, (n, P, P, 3), levels, torch.uint8)
    l8o = _new((n, P, P), levels, torch.uint8) if want_l8 else None
    _call('vpho_photo_clahe_apply_u8', levels, clip, l8, lut, n, P, out, l8o)
    return (out, l8o) if want_l8 else out


def _photo_rows(name, what, t, shape):
    if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32):
        raise VphoError(f'{name}: {what} must be a {shape} float32 tensor')


def photo_grey_sum(levels, colour=None):
    """(n) int64: the sum over each image of the grey level after the shift and brightness of ``colour`` (n,5) (vpho_photo_grey_sum_u8);
    integer adds only, the same bits in every run"""
    n, P = _photo_levels('photo_grey_sum', levels)
    _photo_rows('photo_grey_sum', 'colour', colour, (n, 5))
    sums = torch.zeros(n, dtype=torch.int64, device=levels.device)
    _call('vpho_photo_grey_sum_u8', levels, colour, n, P, sums)
    return sums


def photo_colour(levels, colour=None, contrast=None, hue=None, sums=None, out=None):
    """shift, brightness, contrast, saturation, hue on levels (vpho_photo_colour_u8).  ``colour`` (n,5) as ``frame_patch`` takes it,
    ``contrast`` (n) factors with ``sums`` (n) int64 of ``photo_grey_sum(levels, colour)``, ``hue`` (n) shifts, 0 = skipped."""
    n, P = _photo_levels('photo_colour', levels)
    _photo_rows('photo_colour', 'colour', colour, (n, 5))
    _photo_rows('photo_colour', 'contrast', contrast, (n,))
    _photo_rows('photo_colour', 'hue', hue, (n,))
    if contrast is not None and (sums is None or tuple(sums.shape) != (n,) or sums.dtype != torch.int64):
        raise VphoError('photo_colour: contrast factors need the (n) int64 grey sums of photo_grey_sum')
    out = _photo_out('photo_colour', out, (n, P, P, 3), levels, torch.uint8)
    _call('vpho_photo_colour_u8', levels, colour, contrast, hue, sums, n, P, out)
    return out


def photo_filter(levels, k1, K1, k2, K2, flip=None, erase=None, key=None, out=None):
    """two K x K filters with reflect-101 borders, then the mirror, normalisation and erasing of ``frame_patch`` -> (n,3,P,P) fp32
    (vpho_photo_filter_f32).  ``k1``, ``k2`` (n,49) fp32 on the device, the K * K weights row-major in front; ``K1``, ``K2``: n host
    integers, odd in 1..7 (anything else is refused here)."""
    n, P = _photo_levels('photo_filter', levels)
    _photo_rows('photo_filter', 'k1', k1, (n, 49))
    _photo_rows('photo_filter', 'k2', k2, (n, 49))
    if k1 is None or k2 is None:
        raise VphoError('photo_filter: both kernels are needed (a gate that is off is the 1 x 1 kernel [1])')
    odd = lambda k: 1 <= k <= 7 and k % 2 == 1
    K1 = _photo_host_ints('photo_filter', 'K1', K1, n, odd, 'odd in 1..7').to(levels.device)
    K2 = _photo_host_ints('photo_filter', 'K2', K2, n, odd, 'odd in 1..7').to(levels.device)
    for name, t, shape in (('flip', flip, (n,)), ('erase', erase, (n, 4, 4)), ('key', key, (n, 2))):
        if t is not None and tuple(t.shape) != shape:
            raise VphoError(f'photo_filter: {name} of shape {tuple(t.shape)}, expected {shape}')
    if erase is not None and key is None:
        raise VphoError('photo_filter: erase rectangles need a Philox key')
    out = _photo_out('photo_filter', out, (n, 3, P, P), levels, torch.float32)
    _call('vpho_photo_filter_f32', levels, k1, K1, k2, K2, flip, erase, key, n, P, out)
    return out


# ----------------------------------------------------------------------------------------------- predictions to pixels (raster.hip)
MeshTable = abi.struct('vpho_mesh_table')
RenderLayer = abi.struct('vpho_render_layer')


class MeshRaster:
    """Triangle meshes to depth and face maps, and the overlay compositor (csrc/raster.hip; the rules are in include/vpho_hip.h).

    ``MeshRaster(meshes, device)``: ``meshes`` is a list of ``(verts_count, faces)``, faces (F,3) integer arrays with indices local to
    their mesh.  Every index is validated HERE, once: the kernels trust the table.  ``raster(verts, mesh_id, K, H, W)`` draws n images
    of one mesh each in ONE launch pair; ``overlay(image, K, hand=..., obj=...)`` composites up to two rasterised layers."""
    MAX_SIDE, MAX_VERTS, MAX_FACES, MAX_MESHES = 2048, 1 << 22, 1 << 24, 1 << 16

    def __init__(self, meshes, device):
        import numpy as np
        meshes = list(meshes)
        if not 1 <= len(meshes) <= self.MAX_MESHES:
            raise VphoError(f'MeshRaster: {len(meshes)} meshes, the table takes 1 .. {self.MAX_MESHES}')
        all_faces, counts, nverts = [], [], []
        for i, (V, faces) in enumerate(meshes):
            faces = np.asarray(faces)
            if faces.dtype.kind not in 'iu':
                raise VphoError(f'MeshRaster: mesh {i}: faces must be an integer array, got {faces.dtype}')
            if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
                raise VphoError(f'MeshRaster: mesh {i}: faces of shape {faces.shape}, expected (F, 3) with F >= 1')
            V = int(V)
            if not 1 <= V <= self.MAX_VERTS:
                raise VphoError(f'MeshRaster: mesh {i}: {V} vertices, the table takes 1 .. {self.MAX_VERTS}')
            faces = faces.astype(np.int64)
            if faces.min() < 0 or faces.max() >= V:
                bad = int(np.flatnonzero(((faces < 0) | (faces >= V)).any(1))[0])
                raise VphoError(f'MeshRaster: mesh {i}: face {bad} = {faces[bad].tolist()} indexes outside the {V} vertices')
            all_faces.append(faces)
            counts.append(len(faces))
            nverts.append(V)
        if sum(counts) > self.MAX_FACES:
            raise VphoError(f'MeshRaster: {sum(counts)} faces in all, the table takes at most {self.MAX_FACES}')
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a).astype(np.int32)).to(device).contiguous()
        self.face_counts, self.vert_counts, self.M, self.device = counts, nverts, len(meshes), torch.device(device)
        self.faces, self.face_offset, self.vert_count = dev(np.concatenate(all_faces)), dev(np.concatenate([[0], np.cumsum(counts)])), dev(nverts)
        self.table = MeshTable(self.faces.data_ptr(), self.face_offset.data_ptr(), self.vert_count.data_ptr(), self.M)

    def mesh_ids(self, mesh_id, n=None):
        """ids as a HOST list (checked against the table) and as an int32 device tensor.  A device tensor is read back (one wait): pass a
        list, a numpy array or a CPU tensor to stay asynchronous."""
        dev_ids = mesh_id if torch.is_tensor(mesh_id) and mesh_id.is_cuda else None
        host = [int(i) for i in (mesh_id.reshape(-1).tolist() if hasattr(mesh_id, 'reshape') else list(mesh_id))]
        if n is not None and len(host) != n:
            raise VphoError(f'MeshRaster: {len(host)} mesh ids for {n} images')
        bad = [i for i in host if not 0 <= i < self.M]
        if bad:
            raise VphoError(f'MeshRaster: mesh_id {bad[0]} lies outside the table of {self.M} meshes')
        if dev_ids is None or dev_ids.dtype != torch.int32 or dev_ids.dim() != 1 or not dev_ids.is_contiguous():
            dev_ids = _ids_to_device(host, self.device)
        return host, dev_ids

    def _check_size(self, who, H, W):
        if not (1 <= int(H) <= self.MAX_SIDE and 1 <= int(W) <= self.MAX_SIDE):
            raise VphoError(f'MeshRaster.{who}: {H} x {W} pixels, the kernels take sides of 1 .. {self.MAX_SIDE}')

    def raster(self, verts, mesh_id, K, H, W, z_near=0.01, back=True):
        """verts (n,Vmax,3) fp32 camera-frame metres, mesh_id n ids into the table, K (n,3,3) -> dict of depth_front, face_front (n,H,W) fp32 /
        int32 and, with ``back``, depth_back, face_back; 'verts', 'mesh_id' and 'K' ride along for ``overlay``.  vpho_mesh_raster_f32."""
        self._check_size('raster', H, W)
        if verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[1] < 1:
            raise VphoError(f'MeshRaster.raster: verts of shape {tuple(verts.shape)}, expected (n, Vmax, 3)')
        n, Vmax = verts.shape[0], verts.shape[1]
        if tuple(K.shape) != (n, 3, 3):
            raise VphoError(f'MeshRaster.raster: K of shape {tuple(K.shape)}, expected {(n, 3, 3)}')
        if not (z_near > 0.0 and z_near < 1e30):
            raise VphoError(f'MeshRaster.raster: z_near = {z_near}, expected a positive finite distance')
        host, ids = self.mesh_ids(mesh_id, n)
        for i in set(host):
            if self.vert_counts[i] > Vmax:
                raise VphoError(f'MeshRaster.raster: mesh {i} has {self.vert_counts[i]} vertices, verts holds {Vmax} per image')
        verts, K = verts.float().contiguous(), K.double().contiguous()
        stride = max([self.face_counts[i] for i in host], default=0)
        size = abi.query('vpho_mesh_raster_bytes', n, stride)
        if size < 0:
            raise VphoError(f'vpho_mesh_raster_bytes: n = {n}, face_stride = {stride}')
        ws = torch.empty(max(size, 16), dtype=torch.uint8, device=verts.device)
        df, ff = _new((n, H, W), verts), _new((n, H, W), verts, torch.int32)
        db, fb = (_new((n, H, W), verts), _new((n, H, W), verts, torch.int32)) if back else (None, None)
        _call('vpho_mesh_raster_f32', C.byref(self.table), verts, Vmax, ids, K, n, H, W, stride, z_near, df, db, ff, fb, ws)
        out = dict(depth_front=df, face_front=ff, verts=verts, mesh_id=ids, mesh_id_host=host, K=K)
        if back:
            out.update(depth_back=db, face_back=fb)
        return out

    def _layer(self, who, layer, n, H, W):
        if layer is None:
            return None, None
        df, ff, verts, ids = layer['depth_front'], layer['face_front'], layer['verts'], layer['mesh_id']
        if tuple(df.shape) != (n, H, W) or tuple(ff.shape) != (n, H, W) or verts.dim() != 3 or verts.shape[0] != n or tuple(ids.shape) != (n,):
            raise VphoError(f'MeshRaster.overlay: the {who} layer has maps {tuple(df.shape)} / {tuple(ff.shape)}, verts {tuple(verts.shape)}, '
                            f'mesh_id {tuple(ids.shape)} for {n} images of {H} x {W}')
        # the face maps name vertices of these meshes: the ids are checked on the host again (a layer built by hand brings them as a list)
        host = layer['mesh_id_host'] if 'mesh_id_host' in layer else self.mesh_ids(ids, n)[0]
        for i in set(host):
            if not 0 <= i < self.M or self.vert_counts[i] > verts.shape[1]:
                raise VphoError(f'MeshRaster.overlay: the {who} layer names mesh {i}, which the table or verts {tuple(verts.shape)} cannot hold')
        r, g, b = [float(c) for c in layer.get('colour', (200.0, 200.0, 200.0))]
        op = float(layer.get('opacity', 1.0))
        if not 0.0 <= op <= 1.0:
            raise VphoError(f'MeshRaster.overlay: the {who} layer has opacity {op}, expected 0 .. 1')
        keep = (df, ff, verts, ids)
        return RenderLayer(_f32p(df), abi.addr(ff, torch.int32), _f32p(verts), abi.addr(ids, torch.int32), self.faces.data_ptr(), self.face_offset.data_ptr(), verts.shape[1], self.M,
                           r, g, b, op), keep

    def overlay(self, image, K, hand=None, obj=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), ambient=0.3, out=None):
        """image (n,3,H,W) fp32 normalised, K (n,3,3); ``hand`` / ``obj``: a dict of ``raster`` (its depth_front, face_front, verts, mesh_id)
        with 'colour' (r, g, b on the 0 .. 255 scale) and 'opacity', or None -> (n,H,W,3) uint8.  vpho_render_overlay_u8."""
        if image.dim() != 4 or image.shape[1] != 3:
            raise VphoError(f'MeshRaster.overlay: image of shape {tuple(image.shape)}, expected (n, 3, H, W)')
        n, _, H, W = image.shape
        self._check_size('overlay', H, W)
        if tuple(K.shape) != (n, 3, 3):
            raise VphoError(f'MeshRaster.overlay: K of shape {tuple(K.shape)}, expected {(n, 3, 3)}')
        if not 0.0 <= float(ambient) <= 1.0:
            raise VphoError(f'MeshRaster.overlay: ambient = {ambient}, expected 0 .. 1')
        image, K = image.float().contiguous(), K.double().contiguous()
        lh, keep_h = self._layer('hand', hand, n, H, W)
        lo, keep_o = self._layer('object', obj, n, H, W)
        if out is None:
            out = _new((n, H, W, 3), image, torch.uint8)
        elif tuple(out.shape) != (n, H, W, 3) or out.dtype != torch.uint8:
            raise VphoError(f'MeshRaster.overlay: out of shape {tuple(out.shape)} / {out.dtype}, expected {(n, H, W, 3)} uint8')
        mean3, std3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
        _call('vpho_render_overlay_u8', image, mean3, std3, K, None if lh is None else C.byref(lh), None if lo is None else C.byref(lo), ambient, n,
              H, W, out)
        del keep_h, keep_o
        return out


# ----------------------------------------------------------------------------------------------- physics branch (training)
def cross_tokens_bwd(dtok, want_hand=True, want_obj=True):
    bs = dtok.shape[0]
    dph = torch.zeros((bs, 8, 8, 256), device=dtok.device) if want_hand else None
    dpo = torch.zeros((bs, 8, 8, 256), device=dtok.device) if want_obj else None
    dge = _new((bs, 512), dtok)
    _call('vpho_cross_tokens_bwd_f32', dtok, bs, dph, dpo, dge)
    return dph, dpo, dge


def layernorm_bwd(x, r, gamma, dy, eps=1e-5):
    E = x.shape[-1]
    dx, gx = torch.empty_like(x), torch.empty_like(x)
    _call('vpho_layernorm_bwd_f32', x, r, gamma, dy, x.numel() // E, E, eps, dx, gx)
    return dx, gx


def mha_bwd(qkv, d_out, S, B, E, nhead, drop=None):
    dqkv = torch.empty_like(qkv)
    need = abi.query('vpho_mha_bwd_workspace_bytes', S, B, nhead)
    if need < 0:
        raise VphoError(f'vpho_mha_bwd_workspace_bytes: bad argument (S={S}, B={B}, nhead={nhead}; at most 1024 positions)')
    ws = torch.empty(need, dtype=torch.uint8, device=qkv.device) if need > 0 else None
    _call('vpho_mha_bwd_ws_f32', qkv, d_out, S, B, E, nhead, drop, dqkv, ws)
    return dqkv


def physics_loss(scale_raw, logits, com, anchor, frame, point, gt_force_local, gravity, gt_com, is_grasped, weights, friction=0.8):
    """-> force_local (bs*32,3), losses (5,) fp64 device [force, gravity, torque, supervised, CoM] (weighted), d scale_raw / d logits / d com"""
    bs = gravity.shape[0]
    fl, dsc, dlg, dcm = _new((bs * 32, 3), com), _new((bs * 32, 1), com), _new((bs * 32, 8), com), _new((bs * 32, 3), com)
    losses, ws = _new((5,), com, torch.float64), _new((bs * 5,), com, torch.float64)
    w5 = (C.c_float * 5)(*[float(w) for w in weights])
    _call('vpho_physics_loss_f32', scale_raw, logits, com, anchor, friction, frame, point, gt_force_local, gravity, gt_com, is_grasped, w5, bs, fl,
          dsc, dlg, dcm, losses, ws)
    return fl, losses, dsc, dlg, dcm


# ----------------------------------------------------------------------------------------------- profiling hooks
PROF_CLASSES = {'conv_igemm_128x128': 0, 'conv_igemm_64x64': 1, 'score_head': 2, 'conv_igemm_128x64': 3,
                'mano_fk': 4, 'obj_physics': 5, 'hand_fuse': 6, 'roi_align': 7, 'resize_bilinear': 8, 'conv_winograd': 9,
                'conv_wgrad_64x64': 10, 'conv_wgrad_128x128': 11, 'force_optim': 12, 'pose_encoder': 13}


_prof_on = False


def prof_enable(name, on=True):
    global _prof_on
    _prof_on = bool(on)
    abi.check(abi.query('vpho_prof_enable', PROF_CLASSES[name], 1 if on else 0))


def prof_collect(name):
    ms, n, fl, by = C.c_double(), C.c_longlong(), C.c_double(), C.c_double()
    abi.check(abi.query('vpho_prof_collect', PROF_CLASSES[name], C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
    return dict(total_ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)
