"""Plain torch restatements of the glue and training leaf kernels (csrc/misc.hip, train_score.hip, train_physics.hip), written from the
formulas in the kernel comments / SURVEY.md / INTEGRATION.md.  TEST INFRASTRUCTURE ONLY: nothing here imports ``vpho_amd.ops``.

Every function computes in the dtype of its tensor arguments, so one definition gives both the float64 reference
(``f(*to64(args))``) and torch's own float32 CPU evaluation of the same formula (``f(*args)``), from which ``bound`` derives a tolerance:

    bound = max(4 * max|f32 - f64|, 4 * 2^-23 * max|f64|)

(4x: a different summation order and the <= 2 ulp device sinf / cosf / expf / powf; the floor of 4 ulp of the largest output covers the
cases where torch happens to be exact).  Layouts are the kernels': NHWC maps, row-major matrices."""
import math

import numpy as np
import torch
import torch.nn.functional as F

ULP = 2.0 ** -23
SENT = 12345.0                                                    # the sentinel of every 'untouched' check
SIGMA_MIN, SIGMA_MAX = 0.01, 50.0


def to64(args):
    return [a.double() if torch.is_tensor(a) and a.is_floating_point() else a for a in args]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ruled(f, args, *scalars, **kw):
    """float64 reference and the rule-based bound(s) of f on the float32 CPU tensors `args`"""
    ref = f(*to64(args), *scalars, **kw)
    return ref, bound(f(*args, *scalars, **kw), ref)


def offset_view(t, off=1):
    """a contiguous device copy of t whose base address is `off` elements past a 16-byte boundary, sentinels around it"""
    buf = torch.full((t.numel() + off + 3,), SENT, device='cuda')
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


def boxes(N, g, kind, dtype=torch.float32):
    """tight boxes and their rectangles: equal, larger (samples fall outside the map) or smaller, with an aspect of their own"""
    x0 = torch.rand(N, 2, generator=g, dtype=dtype) * 50
    wh = 40 + torch.rand(N, 2, generator=g, dtype=dtype) * 60
    bbox = torch.cat([x0, x0 + wh], 1).contiguous()
    if kind == 'equal':
        return bbox, bbox.clone()
    c, half = x0 + wh / 2, wh / 2 * torch.tensor({'larger': (1.7, 1.25), 'smaller': (0.6, 0.85)}[kind], dtype=dtype)
    return bbox, torch.cat([c - half, c + half], 1).contiguous()


def bound(f32, f64):
    """the tolerance rule of the module docstring for one output (tensors, or tuples of tensors -> list of bounds)"""
    if isinstance(f64, (tuple, list)):
        return [bound(a, b) for a, b in zip(f32, f64)]
    f64 = f64.double()
    err = float((f32.double() - f64).abs().max()) if f64.numel() else 0.0
    return max(4.0 * err, 4.0 * ULP * float(f64.abs().max()))


def worst(got, ref):
    return float((got.detach().double().cpu() - ref.double()).abs().max())


def check(name, got, ref64, tol):
    """assert max|got - ref64| <= tol; the figures are printed (``pytest -rP`` / ``-s`` shows them: the table of docs/LOG.md)"""
    err = worst(got, ref64)
    line = f'LEAF {name}: worst {err:.3e} bound {tol:.3e}'
    print(line)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), name
    assert err <= tol, line


def bits_equal(a, b):
    """bit-for-bit (distinguishes -0.0 from 0.0, equal NaN payloads compare equal)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


# ------------------------------------------------------------------------------------------------ layout, pooling, resize
def nchw_to_nhwc(x, ld=None):
    N, C, H, W = x.shape
    y = x.new_zeros((N, H, W, C if ld is None else ld))
    y[..., :C] = x.permute(0, 2, 3, 1)
    return y


def nhwc_to_nchw(x, channels=None):
    return x[..., :x.shape[-1] if channels is None else channels].permute(0, 3, 1, 2).contiguous()


def maxpool_nhwc(x, k, stride, pad):
    return F.max_pool2d(x.permute(0, 3, 1, 2), k, stride, pad).permute(0, 2, 3, 1).contiguous()


def resize_bilinear_nhwc(x, OH, OW, channels=None):
    x = x[..., :x.shape[-1] if channels is None else channels]
    return F.interpolate(x.permute(0, 3, 1, 2), size=(OH, OW), mode='bilinear', align_corners=False).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ heat-map re-alignment (quirk Q2)
def _rel(bbox, rect):
    return (rect[:, 2] - rect[:, 0]) / (bbox[:, 2] - bbox[:, 0]), (rect[:, 3] - rect[:, 1]) / (bbox[:, 3] - bbox[:, 1])


def _flip_last_spatial(out, flip):
    if flip is None:
        return out
    return torch.where(flip.bool().view(-1, 1, 1, 1), out.flip(2), out)


def align_heatmap_gather(hm, bbox, rect, flip=None):
    """out[b,i,j,c] = bilinear_zero(hm[b], x = (i/(S-1)*2-1)*rel_w, y = (j/(S-1)*2-1)*rel_h): the FIRST spatial index of the output walks
    x (the map's LAST spatial axis) -- the reference's axis swap --, then the optional flip along j.  hm (N,S,S,C) NHWC."""
    N, S, _, C = hm.shape
    relw, relh = _rel(bbox, rect)
    lin = torch.arange(S, dtype=hm.dtype) / (S - 1) * 2 - 1
    ix = ((lin[None, :] * relw[:, None] + 1) * S - 1) / 2             # (N,S) over i
    iy = ((lin[None, :] * relh[:, None] + 1) * S - 1) / 2             # (N,S) over j
    x0, y0 = torch.floor(ix), torch.floor(iy)
    tx, ty = (ix - x0)[:, :, None, None], (iy - y0)[:, None, :, None]
    x0, y0 = x0.long(), y0.long()
    n = torch.arange(N)[:, None, None]

    def at(yy, xx):                                                    # yy (N,S) over j, xx (N,S) over i -> (N,S_i,S_j,C)
        ok = ((yy >= 0) & (yy < S))[:, None, :] & ((xx >= 0) & (xx < S))[:, :, None]
        v = hm[n, yy.clamp(0, S - 1)[:, None, :], xx.clamp(0, S - 1)[:, :, None]]
        return v * ok[..., None].to(hm.dtype)

    out = (at(y0, x0) * (1 - tx) * (1 - ty) + at(y0, x0 + 1) * tx * (1 - ty) + at(y0 + 1, x0) * (1 - tx) * ty + at(y0 + 1, x0 + 1) * tx * ty)
    return _flip_last_spatial(out, flip)


def align_heatmap_grid_sample(hm, bbox, rect, flip=None):
    """the same through F.grid_sample(padding_mode='zeros', align_corners=False) on the swapped grid"""
    N, S, _, C = hm.shape
    relw, relh = _rel(bbox, rect)
    lin = torch.arange(S, dtype=hm.dtype) / (S - 1) * 2 - 1
    gx = (lin[None, :] * relw[:, None])[:, :, None].expand(N, S, S)   # x depends on the first output index
    gy = (lin[None, :] * relh[:, None])[:, None, :].expand(N, S, S)   # y on the second
    out = F.grid_sample(hm.permute(0, 3, 1, 2), torch.stack([gx, gy], -1), mode='bilinear', padding_mode='zeros', align_corners=False)
    return _flip_last_spatial(out.permute(0, 2, 3, 1).contiguous(), flip)


# ------------------------------------------------------------------------------------------------ cross-module tokens
def nerf_embed(g, flip_x=None):
    """[g, sin(g 2^0), cos(g 2^0), ..., sin(g 2^9), cos(g 2^9)] -> 63 columns + one zero column; flip_x negates g[:, 0] first"""
    if flip_x is not None:
        g = torch.cat([torch.where(flip_x.bool()[:, None], -g[:, :1], g[:, :1]), g[:, 1:]], 1)
    outs = [g]
    for k in range(10):
        outs += [torch.sin(g * 2.0 ** k), torch.cos(g * 2.0 ** k)]
    return torch.cat(outs + [g.new_zeros(g.shape[0], 1)], 1)


def cross_tokens(ph, po, ge, pe):
    """ph, po (bs,8,8,256) NHWC; token n of a stream = channels 8n..8n+7 of the NCHW map flattened (.view(bs,32,-1)); token 64 = the
    gravity embedding; + pe[b] (the positional code is indexed by the BATCH position)"""
    bs = ph.shape[0]
    tok = lambda p: p.permute(0, 3, 1, 2).reshape(bs, 32, 512)
    return torch.cat([tok(ph), tok(po), ge[:, None]], 1) + pe[:bs, None]


def cross_tokens_bwd(dtok):
    """exact adjoint: (d proj_hand, d proj_obj) NHWC, d gravity embedding"""
    bs = dtok.shape[0]
    back = lambda t: t.reshape(bs, 256, 8, 8).permute(0, 2, 3, 1).contiguous()
    return back(dtok[:, :32]), back(dtok[:, 32:64]), dtok[:, 64].contiguous()


def add_layernorm(x, r, gamma, beta, eps=1e-5):
    return F.layer_norm(x + r, (x.shape[-1],), gamma, beta, eps)


def layernorm_bwd(x, r, gamma, dy, eps=1e-5):
    """-> dx (autograd of LayerNorm(x + r) * gamma + beta w.r.t. x), dy * xhat, d gamma, d beta"""
    E = x.shape[-1]
    xx, g = x.detach().clone().requires_grad_(True), gamma.detach().clone().requires_grad_(True)
    b = torch.zeros_like(gamma).requires_grad_(True)
    y = F.layer_norm(xx + r, (E,), g, b, eps)
    dx, dg, db = torch.autograd.grad((y * dy).sum(), [xx, g, b])
    s = (x + r).detach()
    xhat = (s - s.mean(-1, keepdim=True)) / torch.sqrt(s.var(-1, unbiased=False, keepdim=True) + eps)
    return dx, dy * xhat, dg, db


def token_rows(rows, group, group_stride, off):
    r = torch.arange(rows)
    return (r // group) * group_stride + r % group + off


def force_local(scale, logits, anchor, rows, group=1, group_stride=1, off_scale=0, off_logits=0, friction=0.8, double_softmax=True):
    """|scale| * normalise(softmax(softmax(logits)) . cone anchors), anchors' xy scaled by the friction coefficient (quirk Q4: the soft-max
    is applied twice); output row r reads token row (r // group) * group_stride + r % group (+ offset)"""
    s = scale[token_rows(rows, group, group_stride, off_scale), 0]
    w = torch.softmax(logits[token_rows(rows, group, group_stride, off_logits), :8], -1)
    if double_softmax:
        w = torch.softmax(w, -1)
    a = anchor * torch.tensor([friction, friction, 1.0], dtype=anchor.dtype)
    d = w @ a
    return d / (d.norm(dim=-1, keepdim=True) + 1e-8) * s.abs()[:, None]


def append_betas(betas, out, rows_per_image):
    out = out.clone()
    rows = out.shape[0]
    out[:, 48:58] = betas[torch.arange(rows) // rows_per_image]
    return out


# ------------------------------------------------------------------------------------------------ score-network training
def dsm_prepare(gt, t, z, Wf, Dp):
    """t (reps,bs), z (reps,bs,D): std = sigma_min (sigma_max / sigma_min)^t, x_t = x0[b] + z std (zero-padded to Dp), emb = [sin, cos](t W 2 pi)"""
    reps, bs = t.shape
    D = gt.shape[1]
    tt = t.reshape(-1)
    std = SIGMA_MIN * (SIGMA_MAX / SIGMA_MIN) ** tt
    xt = gt.new_zeros((reps * bs, Dp))
    xt[:, :D] = gt.repeat(reps, 1) + z.reshape(reps * bs, D) * std[:, None]
    a = tt[:, None] * Wf[None, :] * 2 * math.pi
    return xt, torch.cat([torch.sin(a), torch.cos(a)], 1), std


def plinear2_fwd(h, w2, b2, std, nheads):
    """score[r, 3n+d] = (b2[n,d] + sum_c h[r, 256n+c] w2[n,c,d]) / (std[r] + 1e-7)"""
    rows = h.shape[0]
    o = torch.einsum('rnc,ncd->rnd', h.view(rows, nheads, 256), w2) + b2[None]
    return o.reshape(rows, 3 * nheads) / (std[:, None] + 1e-7)


def plinear2_bwd(pre, dout, w2, nheads):
    """autograd through out = relu(pre) . w2 + b2 with the seed dout: d pre, d w2, d b2"""
    rows = pre.shape[0]
    p, w = pre.detach().clone().requires_grad_(True), w2.detach().clone().requires_grad_(True)
    b = w2.new_zeros((nheads, 3)).requires_grad_(True)
    o = torch.einsum('rnc,ncd->rnd', torch.relu(p).view(rows, nheads, 256), w) + b[None]
    return torch.autograd.grad((o.reshape(rows, 3 * nheads) * dout).sum(), [p, w, b])


def dsm_loss(out, z, std, batch_times_reps):
    """out = the UN-normalised head output (score = out / (std + 1e-7)); target = -z std / std^2, weight std^2;
    loss = sum w (score - target)^2 / batch_times_reps; -> score, loss, d loss / d out"""
    o = out.detach().clone().requires_grad_(True)
    sd = std[:, None]
    score = o / (sd + 1e-7)
    loss = (sd ** 2 * (score - (-z * sd / sd ** 2)) ** 2).sum() / batch_times_reps
    return score.detach(), loss.detach(), torch.autograd.grad(loss, o)[0]


def dsm_loss_from_score(score, z, std, batch_times_reps):
    """the loss and the kernel's seed gradient 2 w (s - target) / count / (std + 1e-7) from a given score"""
    sd = std[:, None]
    diff = score - (-z * sd / sd ** 2)
    return (sd ** 2 * diff ** 2).sum() / batch_times_reps, 2 * sd ** 2 * diff / batch_times_reps / (sd + 1e-7)


def mse_loss(pd, gt, weight=1.0):
    p = pd.detach().clone().requires_grad_(True)
    loss = weight * F.mse_loss(p, gt)
    return loss.detach(), torch.autograd.grad(loss, p)[0]


def relu_bwd(dy, y):
    return torch.where(y > 0, dy, torch.zeros_like(dy))


def sum_repeats_f32(x, c_off, bs, reps, cols):
    """the kernel's own order: fp32, repeats added left to right starting from 0"""
    s = torch.zeros((bs, cols), dtype=torch.float32)
    for r in range(reps):
        s = s + x[r * bs:(r + 1) * bs, c_off:c_off + cols].float()
    return s


def transpose(x, pad_to=4):
    rows, cols = x.shape
    y = x.new_zeros((cols, (rows + pad_to - 1) // pad_to * pad_to))
    y[:, :rows] = x.t()
    return y


def im2col_t(x, kh, kw, stride, pad_y, pad_x, cin=None):
    """x (N,H,W,ld) NHWC -> (kh*kw*cin, P padded to a multiple of 4), row (r*kw+s)*cin + ci, column p = (n*OH+oy)*OW+ox, via F.unfold"""
    N, H, W, ld = x.shape
    cin = ld if cin is None else cin
    u = F.unfold(x[..., :cin].permute(0, 3, 1, 2), (kh, kw), padding=(pad_y, pad_x), stride=stride)       # (N, cin*kh*kw, L), row ci*kh*kw + tap
    L = u.shape[-1]
    u = u.view(N, cin, kh * kw, L).permute(2, 1, 0, 3).reshape(kh * kw * cin, N * L)
    out = x.new_zeros((kh * kw * cin, (N * L + 3) // 4 * 4))
    out[:, :N * L] = u
    return out


def lrelu_bwd(dy, y, slope):
    return torch.where(y > 0, dy, dy * slope)


def add_lrelu(a, b, slope):
    t = a + b
    return torch.where(t > 0, t, t * slope)


def single_rounding(f, args, *scalars):
    """f evaluated in float64 on float32 inputs and rounded once: for ONE +, -, *, / per output float64 -> float32 double rounding is
    innocuous (53 >= 2 * 24 + 2), so this is the IEEE float32 result bit for bit"""
    return f(*to64(args), *scalars).float()


def add_lrelu_f32(a, b, slope):
    """two roundings, each reproduced exactly: t = fl(a + b), then fl(t * fl(slope))"""
    t = (a.double() + b.double()).float()
    return torch.where(t > 0, t, (t.double() * float(np.float32(slope))).float())


def lrelu_bwd_f32(dy, y, slope):
    return torch.where(y > 0, dy, (dy.double() * float(np.float32(slope))).float())


def f32r(v):
    """a python scalar as the kernel receives it (ctypes c_float)"""
    return float(np.float32(v))


def adamw(param, grad, m, v, step, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0):
    """torch.optim.AdamW (step `step`, resumed from the saved moments m, v) in the dtype of `param`; the hyper-parameters are the float32
    values the kernel receives.  -> new (param, m, v)"""
    p = param.detach().clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=f32r(lr), betas=(f32r(beta1), f32r(beta2)), eps=f32r(eps), weight_decay=f32r(weight_decay), foreach=False)
    p.grad = grad.detach().clone() * f32r(grad_scale)
    opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.detach().clone(), exp_avg_sq=v.detach().clone())
    opt.step()
    st = opt.state[p]
    return p.detach(), st['exp_avg'], st['exp_avg_sq']


def adamw_formula(param, grad, m, v, step, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0):
    """the same update written out (decoupled decay, bias-corrected moments)"""
    g = grad * grad_scale
    param = param * (1 - lr * weight_decay)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    return param - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps)), m, v


# ------------------------------------------------------------------------------------------------ physics losses
PHYS_LOSSES = ('force', 'gravity', 'torque', 'supervised', 'CoM')


def physics_losses(scale_raw, logits, com, anchor, frame, point, gt_local, gravity, gt_com, grasped, weights, friction=0.8):
    """scale_raw (bs*32,1), logits (bs*32,8), com (bs*32,3), anchor (8,3), frame (bs,32,3,3) [j][i], point (bs,32,3), gt_local (bs,32,3),
    gravity (bs,3), gt_com (bs,3), grasped (bs,) -> force_local (bs*32,3), the five WEIGHTED losses (5,):
      force      mean_b (grasped |sum_a f_global + g|)^2          gravity  mean_b (grasped (sum_a f_global . g + 1))^2
      torque     mean_b (grasped |sum_a (point - gt_com) x f_global|)^2
      supervised mse(force_local, gt_local)                       CoM      mse(com, gt_com repeated over the 32 anchors)
    with f_global[j] = sum_i force_local[i] frame[j][i]"""
    bs = gravity.shape[0]
    fl = force_local(scale_raw, logits, anchor, bs * 32, friction=friction)
    fg = torch.einsum('bai,baji->baj', fl.view(bs, 32, 3), frame)
    return fl, five_losses(fl, fg, com, point, gt_local, gravity, gt_com, grasped, weights)


def five_losses(fl, fg, com, point, gt_local, gravity, gt_com, grasped, weights):
    """the five weighted losses from the local forces fl (bs*32,3) and the global forces fg (bs,32,3)"""
    bs = gravity.shape[0]
    gr = grasped.to(fl.dtype)
    Fs = fg.sum(1)
    tq = torch.cross(point - gt_com[:, None], fg, dim=-1).sum(1)
    w = [float(x) for x in weights]
    L = torch.stack([w[0] * (gr ** 2 * ((Fs + gravity) ** 2).sum(-1)).mean(),
                     w[1] * (gr ** 2 * ((Fs * gravity).sum(-1) + 1) ** 2).mean(),
                     w[2] * (gr ** 2 * (tq ** 2).sum(-1)).mean(),
                     w[3] * F.mse_loss(fl.view(bs, 32, 3), gt_local),
                     w[4] * F.mse_loss(com.view(bs, 32, 3), gt_com[:, None].expand(bs, 32, 3))])
    return L


def physics_loss(scale_raw, logits, com, *rest, **kw):
    """-> force_local, losses (5,), and the gradient of their sum w.r.t. scale_raw, logits, com (autograd)"""
    s, l, c = (t.detach().clone().requires_grad_(True) for t in (scale_raw, logits, com))
    fl, L = physics_losses(s, l, c, *rest, **kw)
    ds, dl, dc = torch.autograd.grad(L.sum(), [s, l, c])
    return fl.detach(), L.detach(), ds, dl, dc
