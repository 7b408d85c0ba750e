"""-m gpu: the kernels of csrc/dense_image.hip and the dense image encoder / decoder as a whole.

Kernel cases call the C-ABI directly, in the conventions of tests/test_gpu_map_probe.py: outputs (and the padding of a matrix
with a leading dimension above its row width) start as NaN, references are fp64 restatements of the same fp32 inputs, gradients
come from fp64 autograd, every tolerance is an element-wise bound computed in fp64 from the inputs - `_EPS` times operation
counts times the magnitudes the kernel rounds (the counts are in the docstrings) - and `_close` prints the worst err/tol ratio.

The whole encoder (rows -> MLP -> ELU -> embed with a leading dimension) and the whole decoder head (MLP -> loss -> backward)
are compared against fp64 torch restatements with the element-wise rule of oracle/conv_reference.py (`check_tensor`: the worst
element's error over the reference's rms stays under ten times what the same restatement in fp32 misses fp64 by, floored at 64
roundings), at the tiny widths and at 16 384 rows, where in_dim 196 takes the row-panel layer and in_dim 294 the generic product.
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle.conv_reference import check_tensor       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_EPS = 2.0 ** -23
NAN = float('nan')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _close(a, b, tol, what=''):
    """|a - b| <= tol element-wise (tol a tensor or a scalar); prints the worst err/tol ratio so runs can report it."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(b)
    err = (a - b).abs()
    bad = ~(err <= tol)                              # NaN in a or b fails
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f'[tol] {what}: max err {float(err.max()) if err.numel() else 0:.3e}, worst err/tol {ratio:.3f}')
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e}, ' \
                          f'worst err/tol {ratio:.3e}'


ROWS = [1, 3, 65]


# ------------------------------------------------------------------------------------------------ dm_dense_image_rows
@pytest.mark.parametrize('cells', [1, 49, 50, 121])
@pytest.mark.parametrize('C', [2, 4, 33])
def test_dense_image_rows(hip, C, cells):
    """Equality is exact: the kernel copies or compares, it rounds nothing.  rows in {1, 3, 65}, planes on and off, float and class
    source, ldo padded by 0 and by 3 (the padding starts as NaN and must stay NaN).  The float source is NOT one-hot (random
    values: it is copied as it is); the class source holds classes outside [0, C) (-1, C, 200), which give a zero column."""
    g = _gen(100 * C + cells)
    for rows in ROWS:
        soft = torch.randn(rows, C, cells, generator=g)
        cls = torch.randint(0, C, (rows, cells), generator=g, dtype=torch.int32)
        cls.view(-1)[::5] = torch.tensor([-1, C, 200], dtype=torch.int32).repeat(cls.numel())[:len(cls.view(-1)[::5])]
        reward, terminal = torch.randn(rows, generator=g), (torch.rand(rows, generator=g) < 0.5).float()
        rd, td = reward.to(DEV), terminal.to(DEV)
        onehot = (cls[:, None, :] == torch.arange(C, dtype=torch.int32)[None, :, None]).float()
        assert float(onehot.sum(1).min()) == 0.0          # an out-of-range class: no class of that cell is set
        for planes in (True, False):
            for pad in (0, 3):
                W = (C + 2 * planes) * cells
                for name, src in (('float', soft), ('class', cls)):
                    out = _nan(rows, W + pad)
                    d = src.to(DEV)
                    hip.call('dm_dense_image_rows', rows, C, cells, hip.fptr(d) if name == 'float' else None,
                             hip.ptr(d) if name == 'class' else None, hip.fptr(rd) if planes else None,
                             hip.fptr(td) if planes else None, hip.fptr(out), W + pad, hip.stream())
                    torch.cuda.synchronize()
                    want = [(soft if name == 'float' else onehot).reshape(rows, C * cells)]
                    if planes:
                        want += [reward[:, None].expand(rows, cells), terminal[:, None].expand(rows, cells)]
                    want = torch.cat(want, 1)
                    what = f'{name} C={C} cells={cells} rows={rows} planes={planes} ldo+{pad}'
                    assert torch.equal(out[:, :W].cpu(), want), what
                    assert torch.isnan(out[:, W:]).all(), what + ': padding written'


# ------------------------------------------------------------------------------------------------ dm_elu_rows_fwd / _bwd
@pytest.mark.parametrize('n', [1, 256, 257])
def test_elu_rows(hip, n):
    """y = x for x > 0 (exact), expm1(x) otherwise: tolerance 4 _EPS |y| (expm1f is accurate to a couple of units in the last place,
    relative also for tiny |x|); x = 0 gives y = 0 exactly.  dx = dy * (y > 0 ? 1 : y + 1) from the fp32 y the kernel is handed:
    one rounding for y + 1, one for the product: 2 _EPS |dx|; y = 0 takes the y + 1 = 1 branch, dx = dy exactly.  rows in
    {1, 3, 65}, leading dimensions padded by 0 and by 5 (NaN padding stays NaN), out of place and in place (x == y, dy == dx)."""
    g = _gen(n)
    for rows in ROWS:
        for pad in (0, 5):
            x = torch.randn(rows, n, generator=g) * 3
            x.view(-1)[::7] = 0.0
            x.view(-1)[3::11] = -20.0 * torch.rand(len(x.view(-1)[3::11]), generator=g)       # down to y = -1 + 2e-9
            x.view(-1)[5::13] *= 1e-6                                                         # tiny |x|: expm1 must not cancel
            xb = torch.full((rows, n + pad), NAN)
            xb[:, :n] = x
            xb = xb.to(DEV)
            y = _nan(rows, n + pad)
            hip.call('dm_elu_rows_fwd', rows, n, hip.fptr(xb), n + pad, hip.fptr(y), n + pad, hip.stream())
            xi = xb.clone()
            hip.call('dm_elu_rows_fwd', rows, n, hip.fptr(xi), n + pad, hip.fptr(xi), n + pad, hip.stream())
            torch.cuda.synchronize()
            xd = x.double()
            ref = torch.where(xd > 0, xd, torch.expm1(xd))
            what = f'n={n} rows={rows} ld+{pad}'
            _close(y[:, :n], ref, 4 * _EPS * ref.abs(), 'elu fwd ' + what)
            assert torch.equal(y[:, :n].cpu()[x > 0], x[x > 0]) and float(y[:, :n].cpu()[x == 0].abs().sum()) == 0.0
            assert torch.isnan(y[:, n:]).all() and torch.equal(xi[:, :n], y[:, :n]) and torch.isnan(xi[:, n:]).all()
            dy = torch.randn(rows, n, generator=g)
            dyb = torch.full((rows, n + pad + 1), NAN)
            dyb[:, :n] = dy
            dyb = dyb.to(DEV)
            dx = _nan(rows, n + pad)
            hip.call('dm_elu_rows_bwd', rows, n, hip.fptr(y), n + pad, hip.fptr(dyb), n + pad + 1, hip.fptr(dx), n + pad, hip.stream())
            di = dyb.clone()
            hip.call('dm_elu_rows_bwd', rows, n, hip.fptr(y), n + pad, hip.fptr(di), n + pad + 1, hip.fptr(di), n + pad + 1, hip.stream())
            torch.cuda.synchronize()
            yd = y[:, :n].double().cpu()
            refd = dy.double() * torch.where(yd > 0, torch.ones_like(yd), yd + 1)
            _close(dx[:, :n], refd, 2 * _EPS * refd.abs(), 'elu bwd ' + what)
            assert torch.equal(dx[:, :n].cpu()[x == 0], dy[x == 0])
            assert torch.isnan(dx[:, n:]).all() and torch.equal(di[:, :n], dx[:, :n]) and torch.isnan(di[:, n:]).all()


# ------------------------------------------------------------------------------------------------ dm_cat_image_loss_mix
SHAPES = [(14, 81), (4, 121), (6, 25), (3, 64), (3, 65), (1, 7), (5, 1)]          # the grid of test_gpu_map_probe.py::test_cat_image_loss
ROWS_I = [(1, 1), (7, 1), (130, 1), (129, 3)]


def _logits(rows, C, cells, seed):
    """randn x 2, a tenth of the rows shifted by +-80 and a tenth scaled x 30 (where an unshifted exp overflows and the target's
    softmax underflows to zero), as test_gpu_map_probe.py::_case draws them."""
    g = _gen(seed)
    x = torch.randn(rows, C, cells, generator=g) * 2
    kind = torch.rand(rows, generator=g)
    sign = torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0)
    x = torch.where((kind < 0.1)[:, None, None], x + (80 * sign)[:, None, None], x)
    x = torch.where(((kind >= 0.1) & (kind < 0.2))[:, None, None], x * 30, x)
    return x.float(), g


def _check_mix(hip, x, target, I, m, pad, what):
    rows, C, cells = x.shape
    n, ld = C * cells, C * cells + pad
    buf = torch.full((rows, ld), NAN)
    buf[:, :n] = x.reshape(rows, n)
    buf, tg = buf.to(DEV), target.to(DEV)
    res = []
    for with_d in (True, True, False):
        loss, dl = _nan(rows), _nan(rows, n)
        hip.call('dm_cat_image_loss_mix', rows, I, C, cells, hip.fptr(buf), ld, hip.ptr(tg), m, hip.fptr(loss),
                 hip.fptr(dl) if with_d else None, hip.stream())
        res.append((loss, dl))
    torch.cuda.synchronize()
    loss, dl = res[0]
    m32 = float(torch.tensor(m, dtype=torch.float32))          # the value the C-ABI receives
    xd = x.double().requires_grad_(True)
    t = target.long().repeat_interleave(I, 0)                 # row r reads target row r // I
    s = torch.softmax(xd, 1)
    st = s.gather(1, t[:, None]).squeeze(1)
    pt = (1 - m32) * st + m32 / C
    ref = -torch.log(pt).sum(-1)
    ref.sum().backward()
    with torch.no_grad():
        mx = xd.max(1).values
        gap = (xd.gather(1, t[:, None]).squeeze(1) - mx).abs()
        w = (1 - m32) * st / pt                                # the weight of s_t in p_t, = the gradient's factor g
        K = 16 + math.ceil(cells / 64)
        tol_loss = _EPS * ((C + 12 + w * gap) + (K + 2) * torch.log(pt).abs()).sum(-1)
        delta = F.one_hot(t, C).permute(0, 2, 1).double()
        tol_d = _EPS * w[:, None] * ((C + 12 + (1 - w) * gap)[:, None] * (s - delta).abs() + (C + 8)) + 1e-37
    assert torch.isfinite(loss).all() and torch.isfinite(dl).all(), what
    _close(loss, ref, tol_loss, 'loss ' + what)
    _close(dl, xd.grad.reshape(rows, n), tol_d.reshape(rows, n), 'dlogits ' + what)
    assert torch.equal(res[1][0], loss) and torch.equal(res[1][1], dl), 'two calls on the same inputs differ'
    assert torch.equal(res[2][0], loss) and torch.isnan(res[2][1]).all(), 'dlogits = NULL changes the loss or writes'


@pytest.mark.parametrize('m', [1e-6, 0.05, 0.5])
@pytest.mark.parametrize('C,cells', SHAPES)
def test_cat_image_loss_mix(hip, C, cells, m):
    """dm_cat_image_loss_mix against fp64, rows / I in {(1,1), (7,1), (130,1), (129,3)}, ld padded by 0 and by 5 (NaN padding).
    Per cell s_t = e_t / z carries the C-term sum, the exp, the reciprocal and the product (C + 6 roundings, relative) and the
    rounding of x_t - max (_EPS |x_t - max|, relative, through the exp); p_t = (1 - m) s_t + m / C adds the roundings of 1 - m,
    m / C, the product and the sum, and takes s_t's error with the weight w = (1 - m) s_t / p_t <= 1; the logarithm turns that
    into an absolute error and rounds at its own magnitude: loss tolerance _EPS x sum_cells (C + 12 + w |x_t - max| + (K + 2)
    |log p_t|), K = 16 + ceil(cells / 64) for the row sum (lane additions, six shuffle levels, up to four LDS partials).
    dlogits_c = g (s_c - delta_ct), g = w: the relative error of g is that of s_t with the weight 1 - w plus the division and
    products, s_c carries C + 8 roundings: tolerance _EPS g ((C + 12 + (1 - w) |x_t - max|) |s_c - delta| + C + 8) (+ 1e-37 where
    s_t underflows to a denormal or zero: g is then below 1e-30 in fp64 as well)."""
    for rows, I in ROWS_I:
        x, g = _logits(rows, C, cells, seed=3000 * C + 10 * cells + rows + I)
        target = torch.randint(0, C, (rows // I, cells), generator=g, dtype=torch.int32)
        for pad in (0, 5):
            _check_mix(hip, x, target, I, m, pad, f'C={C} cells={cells} rows={rows} I={I} m={m} ld+{pad}')


@pytest.mark.parametrize('m', [1e-6, 0.05, 0.5])
def test_cat_image_loss_mix_with_an_underflowing_target(hip, m):
    """The target's logit lies 60 below the maximum in every cell (and 120 below in one row, where expf underflows to zero):
    s_t ~ 1e-26 vanishes beside m / C, p_t ~ m / C; loss and gradient must stay finite and within the bound of the case above."""
    rows, C, cells = 5, 4, 49
    x = torch.randn(rows, C, cells, generator=_gen(9)).float()
    target = torch.randint(0, C, (rows, cells), generator=_gen(10), dtype=torch.int32)
    hot = torch.nn.functional.one_hot(target.long(), C).permute(0, 2, 1).bool()
    x = torch.where(hot, x.amax(1, keepdim=True) - 60.0, x)
    x[4] = torch.where(hot[4], x[4].amax(0, keepdim=True) - 120.0, x[4])
    _check_mix(hip, x, target, 1, m, 0, f'target logit 60 below the maximum, m={m}')
    out_of_range = target.clone()
    out_of_range[0, ::3] = C
    out_of_range[1, ::4] = -1
    loss, dl = _nan(rows), _nan(rows, C * cells)
    xg, tg = x.reshape(rows, -1).to(DEV), out_of_range.to(DEV)
    hip.call('dm_cat_image_loss_mix', rows, 1, C, cells, hip.fptr(xg), C * cells, hip.ptr(tg), m, hip.fptr(loss), hip.fptr(dl), hip.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(dl).all()
    assert float(dl.view(rows, C, cells)[0, :, ::3].abs().max()) == 0.0, 'a target outside [0, C) has a zero gradient'


# ------------------------------------------------------------------------------------------------ encoder and decoder as a whole
def _wm(image_size=7, image_channels=4, reward_input=True, enc_layers=3, dec_layers=2, min_prob=0.0, seed=0):
    from pydreamer_amd import config
    from pydreamer_amd.models import WorldModel
    conf = config.load_config('defaults', 'minigrid', deter_dim=64, hidden_dim=64, stoch_dim=8, stoch_discrete=8, image_size=image_size,
                              image_channels=image_channels, reward_input=reward_input, image_encoder_layers=enc_layers,
                              image_decoder_layers=dec_layers, image_decoder_min_prob=min_prob)
    torch.manual_seed(seed)
    wm = WorldModel(conf)
    with torch.no_grad():          # tf2 init leaves zero biases and unit LayerNorm: give every parameter a value that matters
        for n, p in wm.named_parameters():
            if n.startswith(('encoder.', 'decoder.image.')) and p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape))
    return conf, wm.to(DEV)


def _mlp_ref(params, x, layers, dtype, elu_out):
    p = [v.detach().to(dtype).cpu().requires_grad_(True) for v in params]
    h = x.to(dtype).cpu().requires_grad_(True)
    x0 = h
    for l in range(layers):
        w, b, g, be = p[4 * l:4 * l + 4]
        h = F.elu(F.layer_norm(h @ w.T + b, (w.shape[0],), g, be, 1e-3))
    h = h @ p[4 * layers].T + p[4 * layers + 1]
    return (F.elu(h) if elu_out else h), p, x0


def _struct(hip, shape_rows, wm, conf):
    shp = wm.shape(1, shape_rows, 1)
    return wm.workspace(shp, torch.device(DEV, torch.cuda.current_device()))


@pytest.mark.parametrize('rows,reward_input,layers', [(15, True, 3), (15, False, 1), (16384, False, 2), (16384, True, 2)])
def test_encoder_against_fp64(hip, rows, reward_input, layers):
    """MultiEncoder.dense_encode (dm_dense_image_rows -> MLP -> dm_elu_rows_fwd into an embed buffer with a leading dimension of 256
    + 8) and its backward (dm_elu_rows_bwd in place, dm_mlp_head_bwd without an input gradient) against fp64 autograd: in_dim 196
    (no planes: a multiple of 4, the row-panel layer at 16 384 rows) and 294 (planes: the generic product)."""
    import ctypes
    conf, wm = _wm(reward_input=reward_input, enc_layers=layers, seed=rows + layers)
    enc = wm.encoder.encoder_image
    assert enc.in_dim == (294 if reward_input else 196)
    g = _gen(rows)
    C, S = conf.image_channels, conf.image_size
    cls = torch.randint(0, C, (rows, S * S), generator=g, dtype=torch.int32)
    onehot = F.one_hot(cls.long(), C).permute(0, 2, 1).float().contiguous()                # (rows, C, cells)
    reward, terminal = torch.tanh(torch.randn(rows, generator=g)), (torch.rand(rows, generator=g) < 0.1).float()
    pr, pt = (reward.to(DEV), terminal.to(DEV)) if reward_input else (None, None)
    ws = _struct(hip, rows, wm, conf)
    embed, embed_i = _nan(rows, 264), _nan(rows, 264)
    x, acts = wm.encoder.dense_encode(onehot.to(DEV), pr, pt, embed, rows, ws, save=True)
    wm.encoder.dense_encode(cls.to(DEV), pr, pt, embed_i, rows, ws, save=False)
    torch.cuda.synchronize()
    assert torch.equal(embed[:, :256], embed_i[:, :256]), 'the class map and its one-hot form give different bits'
    assert torch.isnan(embed[:, 256:]).all(), 'embed padding written'
    xin = torch.cat([onehot.reshape(rows, -1)] + ([reward[:, None].expand(rows, S * S), terminal[:, None].expand(rows, S * S)]
                                                  if reward_input else []), 1)
    assert torch.equal(x.cpu(), xin)
    params = list(enc.parameters())
    dembed = torch.randn(rows, 256, generator=g) / rows
    refs = {}
    for dtype in (torch.float64, torch.float32):
        y, p, _ = _mlp_ref(params, xin, layers, dtype, elu_out=True)
        (y * dembed.to(dtype)).sum().backward()
        refs[dtype] = (y.detach(), [v.grad for v in p])
    report = []
    check_tensor('embed', embed[:, :256].cpu(), refs[torch.float64][0], refs[torch.float32][0], ('row', 'col'), report)
    # backward, as WorldModel._backward runs it
    E = 264
    dbuf = _nan(rows, E)
    dbuf[:, :256] = dembed.to(DEV)
    grads = [torch.full_like(p, NAN) for p in params]
    gof = {id(p): gr for p, gr in zip(params, grads)}
    hip.call('dm_elu_rows_bwd', rows, 256, hip.fptr(embed), E, hip.fptr(dbuf), E, hip.fptr(dbuf), E, hip.stream())
    dpre = dbuf[:, :256].contiguous()
    st, gs = enc.struct(), enc.grad_struct(gof)
    hip.call('dm_mlp_head_bwd', rows, enc.in_dim, enc.hidden_dim, enc.hidden_layers, enc.out_dim, hip.fptr(x), enc.in_dim,
             ctypes.byref(st), hip.fptr(acts), hip.fptr(dpre), ctypes.byref(gs), None, 0, 0, hip.ptr(ws), ws.numel(), hip.stream())
    torch.cuda.synchronize()
    for (n, _), got, r64, r32 in zip(enc.named_parameters(), grads, refs[torch.float64][1], refs[torch.float32][1]):
        check_tensor('d ' + n, got.cpu(), r64, r32, tuple('ab'[:got.dim()]), report)
    for name, err, err32, bar in report:
        print(f'[bar] encoder rows={rows} in_dim={enc.in_dim} {name}: err {err:.3e} ref32 {err32:.3e} bar {bar:.3e} ratio {err / bar:.3f}')


@pytest.mark.parametrize('rows,min_prob', [(15, 0.0), (15, 0.05), (16384, 0.0), (16384, 0.05)])
def test_decoder_head_against_fp64(hip, rows, min_prob):
    """The image decoder as WorldModel runs it - MLP.fwd on the feature rows, CatImageDecoder.loss, the scaled output gradient
    through dm_mlp_head_bwd with the input gradient ACCUMULATED into a pre-filled buffer, CatImageDecoder.logp - against fp64
    autograd of CatImageDecoder.training_step (decoders.py:219-254)."""
    import ctypes
    conf, wm = _wm(min_prob=min_prob, seed=rows)
    dec = wm.decoder.image
    C, cells, F_ = conf.image_channels, conf.image_size ** 2, wm.features_dim
    g = _gen(rows + 1)
    feat = torch.cat([torch.tanh(torch.randn(rows, conf.deter_dim, generator=g)),
                      F.one_hot(torch.randint(0, 8, (rows, 8), generator=g), 8).float().reshape(rows, 64)], 1)
    target = torch.randint(0, C, (rows, cells), generator=g, dtype=torch.int32)
    ws = _struct(hip, rows, wm, conf)
    fd, tg = feat.to(DEV), target.to(DEV)
    logits, acts = dec.fwd(fd, F_, rows, ws, save_acts=True)
    loss, dlogits = _nan(rows), _nan(rows, C * cells)
    dec.loss(logits, tg, rows, loss, dlogits)
    logp = dec.logp(logits, tg, rows)
    scale = 1.0 / rows
    hip.call('dm_scale_inplace', hip.fptr(dlogits), dlogits.numel(), hip.fptr(torch.full((1,), scale, device=DEV)), hip.stream())
    params = list(dec.parameters())
    grads = [torch.full_like(p, NAN) for p in params]
    gof = {id(p): gr for p, gr in zip(params, grads)}
    base = torch.randn(rows, F_, generator=g) / rows
    dfeat = base.to(DEV)
    st, gs = dec.struct(), dec.grad_struct(gof)
    hip.call('dm_mlp_head_bwd', rows, F_, dec.hidden_dim, dec.hidden_layers, dec.out_dim, hip.fptr(fd), F_, ctypes.byref(st),
             hip.fptr(acts), hip.fptr(dlogits), ctypes.byref(gs), hip.fptr(dfeat), F_, 1, hip.ptr(ws), ws.numel(), hip.stream())
    torch.cuda.synchronize()
    refs = {}
    m32 = float(torch.tensor(min_prob, dtype=torch.float32))
    for dtype in (torch.float64, torch.float32):
        y, p, x0 = _mlp_ref(params, feat, dec.hidden_layers, dtype, elu_out=False)
        y3 = y.view(rows, C, cells)
        if min_prob == 0:
            l = F.nll_loss(F.log_softmax(y3, 1), target.long(), reduction='none').sum(-1)
        else:
            prob = (1.0 - m32) * F.softmax(y3, 1) + m32 * (1.0 / C)
            l = F.nll_loss(prob.log(), target.long(), reduction='none').sum(-1)
        (l.sum() * scale).backward()
        refs[dtype] = dict(logits=y.detach(), loss=l.detach(), logp=F.log_softmax(y3, 1).detach(), dfeat=x0.grad + base.to(dtype),
                           grads=[v.grad for v in p])
    r64, r32 = refs[torch.float64], refs[torch.float32]
    report = []
    check_tensor('logits', logits.cpu(), r64['logits'], r32['logits'], ('row', 'col'), report)
    check_tensor('loss', loss.cpu(), r64['loss'], r32['loss'], ('row',), report)
    check_tensor('logp', logp.cpu(), r64['logp'], r32['logp'], ('row', 'class', 'cell'), report)
    check_tensor('dfeat', dfeat.cpu(), r64['dfeat'], r32['dfeat'], ('row', 'col'), report)
    for (n, _), got, a, b in zip(dec.named_parameters(), grads, r64['grads'], r32['grads']):
        check_tensor('d ' + n, got.cpu(), a, b, tuple('ab'[:got.dim()]), report)
    for name, err, err32, bar in report:
        print(f'[bar] decoder rows={rows} min_prob={min_prob} {name}: err {err:.3e} ref32 {err32:.3e} bar {bar:.3e} ratio {err / bar:.3f}')
