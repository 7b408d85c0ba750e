"""-m gpu: the map probe (probe_model='map').

Kernel cases call the C-ABI of csrc/cat_image.hip directly; conventions of test_gpu_distributions.py: outputs start as NaN (the
padding of an ld > C*cells logit matrix is NaN too, so a read past a row's C*cells logits poisons the result), references are fp64
restatements of the same fp32 inputs written with torch.logsumexp / log_softmax, gradients come from fp64 autograd, and every
tolerance is an element-wise bound computed in fp64 from the inputs - `_EPS` times operation counts times the magnitudes the
kernel rounds (the counts are in the docstrings).  `_close` prints the worst err/tol ratio.

Step cases run the whole model against the reference-written fixtures tests/golden/tiny_map_probe.npz and
tiny_map_probe_iwae.npz (scripts/gen_map_probe_golden.py) with the bars tests/test_gpu_obs_inputs.py applies to the vecobs
head, check bit-identity over `overlap_backward`, independence of the other three losses from the probe, and the head alone at
the miniworld widths (hidden 1024, 14 x 9 x 9 logits) against an fp64 torch restatement.
"""
import ast
import math
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_form_params as CFP                     # noqa: E402
from oracle import dreamer_oracle as O               # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
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


# ------------------------------------------------------------------------------------------------ kernel cases
SHAPES = [(14, 81), (4, 121), (6, 25), (3, 64), (3, 65), (1, 7), (5, 1)]
ROWS = [(1, 1), (7, 1), (130, 1), (129, 3)]
MIN_GAP = 1e-3


def _agg_logp(x):
    """decoders.py:247-251 in fp64: x (groups, I, C, cells) -> (groups, C, cells)."""
    y = x - torch.logsumexp(x, 2, keepdim=True)
    a = torch.logsumexp(y, 1)
    return a - torch.logsumexp(a, 1, keepdim=True)


def _case(rows, I, C, cells, pad, seed):
    """Logits randn x 2, a tenth of the rows shifted by +-80 and a tenth scaled x 30 (where an unshifted exp overflows), in a
    NaN-padded (rows, C*cells + pad) matrix.  Every cell's top-two gap of the I-aggregated fp64 log-probabilities is at least
    MIN_GAP BY CONSTRUCTION: 0.01 is added to the leading class's logit (in all I rows) of any cell with a smaller gap, and the
    check is repeated with the amount doubled until every cell passes - one addition of 0.01 does not move a cell whose tie is
    between classes that two different rows of the group hold with probability one (x 30 rows: the amount then has to grow to
    the spread of those rows' logits).  No case and no cell is excluded from the
    exact-accuracy demand."""
    g = _gen(seed)
    groups, n = rows // I, C * cells
    x = torch.randn(rows, C, cells, generator=g) * 2
    kind = torch.rand(rows, generator=g)
    sign = torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0)
    x = torch.where((kind < 0.1)[:, None, None], x + (80 * sign)[:, None, None], x)
    x = torch.where(((kind >= 0.1) & (kind < 0.2))[:, None, None], x * 30, x)
    x = x.float()
    step = 0.01
    while C > 1:
        top = _agg_logp(x.double().view(groups, I, C, cells)).topk(2, dim=1)
        small = (top.values[:, 0] - top.values[:, 1]) < MIN_GAP                      # (groups, cells)
        if not small.any():
            break
        assert step < 1000, 'the construction did not converge'
        bump = torch.zeros(groups, C, cells).scatter_(1, top.indices[:, :1], small[:, None].float() * step)
        x = (x.view(groups, I, C, cells) + bump[:, None]).view(rows, C, cells).float()
        step *= 2
    target = torch.randint(0, C, (groups, cells), generator=g, dtype=torch.int32)
    seen = (torch.rand(groups, cells, generator=g) < 0.5).to(torch.int32)
    seen[0] = 0                                       # a frame without a seen cell: acc_seen is NaN there
    if groups > 1:
        seen[1] = 1                                   # a frame seen everywhere: acc_seen equals acc there
    buf = torch.full((rows, n + pad), NAN)
    buf[:, :n] = x.view(rows, n)
    return buf.to(DEV), x, target.to(DEV), seen.to(DEV)


@pytest.mark.parametrize('pad', [0, 5])
@pytest.mark.parametrize('rows,I', ROWS)
@pytest.mark.parametrize('C,cells', SHAPES)
def test_cat_image_loss(hip, C, cells, rows, I, pad):
    """dm_cat_image_loss against fp64.  loss[r]: tolerance _EPS x (C + K) x sum_cells (1 + |max| + |lse - max| + |x_t|), K = 16 +
    ceil(cells / 64): per cell the C-term sum of exponentials (relative C _EPS on a sum >= 1, hence the 1: the logarithm turns it
    into an absolute error), the roundings of x - max, log, max + log and - x_t (each at most _EPS times one of the magnitudes
    listed), then at most ceil(cells / 64) additions per lane, six shuffle levels and up to four LDS partials for the row sum.
    dlogits in [-1, 1]: (C + 8) _EPS - the C-term sum, exp, the reciprocal, the product and the subtraction of the one-hot; the
    rounding of x - max moves exp by _EPS |x - max| p <= 0.37 _EPS."""
    buf, x, target, _ = _case(rows, I, C, cells, pad, seed=1000 * C + 10 * cells + rows + I)
    n, ld = C * cells, C * cells + pad
    loss, dl = _nan(rows), _nan(rows, n)
    hip.call('dm_cat_image_loss', rows, I, C, cells, hip.fptr(buf), ld, hip.ptr(target), hip.fptr(loss), hip.fptr(dl), hip.stream())
    loss2, dl2, loss3 = _nan(rows), _nan(rows, n), _nan(rows)
    hip.call('dm_cat_image_loss', rows, I, C, cells, hip.fptr(buf), ld, hip.ptr(target), hip.fptr(loss2), hip.fptr(dl2), hip.stream())
    hip.call('dm_cat_image_loss', rows, I, C, cells, hip.fptr(buf), ld, hip.ptr(target), hip.fptr(loss3), None, hip.stream())
    torch.cuda.synchronize()
    xd = x.double().requires_grad_(True)                                           # (rows, C, cells)
    tg = target.cpu().long().repeat_interleave(I, 0)                               # row r reads target row r // I
    lse = torch.logsumexp(xd, 1)
    xt = xd.gather(1, tg[:, None]).squeeze(1)
    ref = (lse - xt).sum(-1)
    ref.sum().backward()
    mx = xd.detach().max(1).values
    mag = (1 + mx.abs() + (lse.detach() - mx).abs() + xt.detach().abs()).sum(-1)
    K = 16 + math.ceil(cells / 64)
    _close(loss, ref, _EPS * (C + K) * mag, f'loss C={C} cells={cells} rows={rows} I={I} ld+{pad}')
    _close(dl, xd.grad.reshape(rows, n), (C + 8) * _EPS, f'dlogits C={C} cells={cells} rows={rows} I={I} ld+{pad}')
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2), 'two calls on the same inputs differ'
    assert torch.equal(loss, loss3), 'dlogits = NULL changes the loss'


@pytest.mark.parametrize('pad', [0, 5])
@pytest.mark.parametrize('rows,I', ROWS)
@pytest.mark.parametrize('C,cells', SHAPES)
def test_cat_image_pred(hip, C, cells, rows, I, pad):
    """dm_cat_image_pred against fp64.  logp[g][c][p]: tolerance _EPS x (3C + 2I + 25 + 2 max_i |lse_i| + max_i |y_ic| + |a_c| + |L| +
    |logp|), y = x - lse_i, a_c = logsumexp_i y, L = logsumexp_c a.  Twice (once through a_c, once through L) the error of
    lse_i - its C-term sum, C + 6 roundings of unit sensitivity, and _EPS |lse_i| - and of the I-term sum behind a logarithm
    (I + 4); the C-term sum of L (C + 4); the roundings of the three subtractions and additions at their own magnitudes.
    acc and acc_seen are demanded EXACTLY: integer counts over cells whose top-two gap is >= 1e-3 by construction, one
    correctly rounded division; acc_seen is NaN for the frame without a seen cell and equals acc for the frame seen everywhere."""
    buf, x, target, seen = _case(rows, I, C, cells, pad, seed=2000 * C + 10 * cells + rows + I)
    groups, ld = rows // I, C * cells + pad
    out = []
    for with_logp in (True, True, False):
        logp, acc, acs = _nan(groups, C, cells), _nan(groups), _nan(groups)
        hip.call('dm_cat_image_pred', groups, I, C, cells, hip.fptr(buf), ld, hip.ptr(target), hip.ptr(seen),
                 hip.fptr(logp) if with_logp else None, hip.fptr(acc), hip.fptr(acs), hip.stream())
        out.append((logp, acc, acs))
    acc_only = _nan(groups)
    hip.call('dm_cat_image_pred', groups, I, C, cells, hip.fptr(buf), ld, hip.ptr(target), None, None, hip.fptr(acc_only), None, hip.stream())
    torch.cuda.synchronize()
    logp, acc, acs = out[0]
    xd = x.double().view(groups, I, C, cells)
    lse = torch.logsumexp(xd, 2, keepdim=True)
    y = xd - lse
    a = torch.logsumexp(y, 1)
    L = torch.logsumexp(a, 1, keepdim=True)
    ref = a - L
    tol = _EPS * (3 * C + 2 * I + 25 + 2 * lse.abs().amax(1) + y.abs().amax(1) + a.abs() + L.abs() + ref.abs())
    _close(logp, ref, tol, f'logp C={C} cells={cells} rows={rows} I={I} ld+{pad}')
    tg, sn = target.cpu().long(), seen.cpu().long()
    hit = (ref.argmax(1) == tg).long()
    ref_acc = hit.sum(-1).float() / torch.tensor(float(cells))
    ref_acs = (hit * sn).sum(-1).float() / sn.sum(-1).float()
    assert torch.equal(acc.cpu(), ref_acc), (acc.cpu(), ref_acc)
    assert torch.isnan(acs[0]) and torch.isnan(ref_acs[0])
    assert torch.equal(torch.nan_to_num(acs.cpu(), nan=-1.0), torch.nan_to_num(ref_acs, nan=-1.0))
    if groups > 1:
        assert float(acs[1]) == float(acc[1])
    for o in out[1:]:
        assert torch.equal(o[1], acc) and torch.equal(torch.nan_to_num(o[2], nan=-1.0), torch.nan_to_num(acs, nan=-1.0))
    assert torch.equal(out[1][0], logp), 'two calls on the same inputs differ'
    assert torch.isnan(out[2][0]).all(), 'logp = NULL: nothing may be written'
    assert torch.equal(acc_only, acc), 'seen = NULL / logp = NULL changes acc'


def test_equal_values_take_the_lowest_class(hip):
    """torch.argmax on exactly equal values returns the first index (decoders.py:221, probes.py:75,79): dm_cat_target_index on a
    soft target whose classes 1 and 3 tie, and the accuracy on logits whose classes 1 and 3 are the same float."""
    C, cells, rows = 5, 70, 3
    soft = torch.rand(rows, C, cells, generator=_gen(1)) * 0.2
    soft[:, 1] = 0.5
    soft[:, 3] = 0.5
    soft[0, 0, :5] = 0.5                              # a three-way tie that class 0 wins
    idx = torch.full((rows, cells), -1, dtype=torch.int32, device=DEV)
    hip.call('dm_cat_target_index', rows, C, cells, hip.fptr(soft.to(DEV)), hip.ptr(idx), hip.stream())
    rnd = torch.randn(33, 7, 130, generator=_gen(2))
    idx2 = torch.full((33, 130), -1, dtype=torch.int32, device=DEV)
    hip.call('dm_cat_target_index', 33, 7, 130, hip.fptr(rnd.to(DEV)), hip.ptr(idx2), hip.stream())
    x = torch.randn(rows, C, cells, generator=_gen(3))
    x[:, 1] = 2.5
    x[:, 3] = 2.5
    x[:, [0, 2, 4]] = x[:, [0, 2, 4]].clamp_max(1.0)
    t1 = torch.full((rows, cells), 1, dtype=torch.int32, device=DEV)
    t3 = torch.full((rows, cells), 3, dtype=torch.int32, device=DEV)
    acc1, acc3 = _nan(rows), _nan(rows)
    xg = x.reshape(rows, C * cells).to(DEV)
    hip.call('dm_cat_image_pred', rows, 1, C, cells, hip.fptr(xg), C * cells, hip.ptr(t1), None, None, hip.fptr(acc1), None, hip.stream())
    hip.call('dm_cat_image_pred', rows, 1, C, cells, hip.fptr(xg), C * cells, hip.ptr(t3), None, None, hip.fptr(acc3), None, hip.stream())
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu().long(), soft.argmax(1)) and int(idx[0, 0]) == 0 and int(idx[1, 0]) == 1
    assert torch.equal(idx2.cpu().long(), rnd.argmax(1))
    assert acc1.tolist() == [1.0] * rows and acc3.tolist() == [0.0] * rows


# ------------------------------------------------------------------------------------------------ the head alone
def _ref_head(params, x, target, C, cells, I, layers):
    """CatImageDecoder.training_step (decoders.py:238-254) on fp64 copies of the parameters: loss_probe and its autograd gradients."""
    p = [v.detach().double().cpu().requires_grad_(True) for v in params]
    h = x.double().cpu()
    for l in range(layers):
        w, b, g, be = p[4 * l:4 * l + 4]
        h = F.elu(F.layer_norm(h @ w.T + b, (w.shape[0],), g, be, 1e-3))
    logits = (h @ p[4 * layers].T + p[4 * layers + 1]).view(-1, C, cells)
    tg = target.cpu().long().repeat_interleave(I, 0)
    loss_tbi = (torch.logsumexp(logits, 1) - logits.gather(1, tg[:, None]).squeeze(1)).sum(-1).view(-1, I)
    loss_tb = -(torch.logsumexp(-loss_tbi, 1) - math.log(I))
    loss = loss_tb.mean()
    loss.backward()
    return loss.detach(), loss_tb.detach(), [v.grad for v in p]


@pytest.mark.parametrize('T,B,I,layers', [(6, 5, 1, 4), (48, 32, 1, 2), (5, 3, 2, 2)])
def test_head_at_miniworld_widths_against_fp64(hip, T, B, I, layers):
    """MapProbeHead alone at the `miniworld` widths (map 14 x 9 x 9, hidden 1024: the MLP's generic GEMM + LayerNorm path at 30,
    1536 and 30 rows) against an fp64 restatement; the bars of the step cases: loss 2e-5 relative, loss_map tensor 1e-4, gradient
    norms 2e-3, full gradients 2e-3 relative L2.  An integer class map gives the same bits as its one-hot form."""
    from pydreamer_amd.models import MapProbeHead
    F_, C, S = 100, 14, 9
    conf = Namespace(map_decoder='dense', map_channels=C, map_size=S, map_hidden_dim=1024, map_hidden_layers=layers, layer_norm=True)
    torch.manual_seed(T)
    head = MapProbeHead(F_ + 4, conf).to(DEV)
    g = _gen(T + B)
    feats = torch.tanh(torch.randn(T, B, I, F_, generator=g)).to(DEV)
    classes = torch.randint(0, C, (T, B, S, S), generator=g)
    obs = dict(map=F.one_hot(classes, C).permute(0, 1, 4, 2, 3).float().contiguous().to(DEV),
               map_coord=torch.randn(T, B, 4, generator=g).to(DEV))
    loss, metrics, tensors = head.training_step(feats, obs)
    loss.backward()
    with torch.no_grad():
        loss_i, _, t_i = head.training_step(feats, dict(obs, map=classes.to(DEV)))
    torch.cuda.synchronize()
    x = torch.cat([feats.cpu(), obs['map_coord'].cpu()[:, :, None].expand(T, B, I, 4)], -1).reshape(T * B * I, F_ + 4)
    params = list(head.decoder.parameters())
    ref, ref_tb, grads = _ref_head(params, x, classes.view(T * B, S * S), C, S * S, I, layers)
    print(f'loss {float(loss):.8g} fp64 {float(ref):.8g}')
    assert abs(float(loss) - float(ref)) < 2e-5 * abs(float(ref))
    assert float(loss_i) == float(loss) and torch.equal(t_i['map_rec'], tensors['map_rec'])
    _close(tensors['loss_map'], ref_tb.view(T, B), 1e-4 * ref_tb.abs().max(), 'loss_map tensor')
    for (n, p), gr in zip(head.decoder.named_parameters(), grads):
        got = p.grad.double().cpu()
        assert abs(float(got.norm()) - float(gr.norm())) <= 2e-3 * float(gr.norm()) + 1e-7, n
        e = float((got - gr).norm() / gr.norm())
        if n in ('model.0.weight', f'model.{3 * layers}.weight'):
            print(f'full gradient {n}: relative L2 error {e:.3e}')
            assert e < 2e-3, (n, e)
    with pytest.raises(RuntimeError):
        loss.backward()


# ------------------------------------------------------------------------------------------------ step cases
def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-12)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _close_rt(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    bound = atol + rtol * b.abs()
    print(f'[tol] {what}: max err {float(err.max()):.3e}, worst err/tol {float((err / bound).max()):.3f}')
    assert not (err > bound).any(), f'{what}: {int((err > bound).sum())}/{err.numel()} mismatches, max err {float(err.max()):.3e}'


def _model(g, **more):
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    model = Dreamer(config.load_config('defaults', 'atari', **{**vars(oconf), **extra, **more}))
    shapes = CFP.shapes_of_fixture(g)
    if more.get('probe_model') == 'none':
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        assert list(shapes)[:-1] == [k for k in CFP.shapes_of_fixture(g) if not k.startswith('probe_model.')]
    assert list(model.state_dict().keys()) == list(shapes.keys())
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)      # one seed per tensor INDEX: wm / ac do not depend on the probe
    return oconf, model.to(DEV)


def _obs(g, pre, oconf, C):
    raw = {k: g[pre + 'in_' + k] for k in ('image_u8', 'action_idx', 'reward', 'terminal', 'reset')}
    obs = {k: v.to(DEV) for k, v in O.preprocess(raw, oconf).items()}
    classes = torch.from_numpy(g[pre + 'in_map_classes'].astype(np.int64))
    obs['map'] = F.one_hot(classes, C).permute(0, 1, 4, 2, 3).float().contiguous().to(DEV)
    obs['map_coord'] = torch.from_numpy(g[pre + 'in_map_coord']).to(DEV)
    obs['map_seen_mask'] = torch.from_numpy(g[pre + 'in_map_seen_mask']).to(DEV)
    noise = {k: torch.from_numpy(g[pre + 'in_' + k]).to(DEV) for k in ('u_post', 'u_act', 'u_prior')}
    return obs, noise


@pytest.mark.parametrize('name,steps', [('tiny_map_probe', 2), ('tiny_map_probe_iwae', 1)])
def test_training_steps_match_the_reference(hip, name, steps):
    """Trainer iterations with carried state on the fixture's inputs and noise.  Bars of tests/test_gpu_obs_inputs.py, unchanged:
    losses 2e-5 relative (or 2e-6), metrics 1e-4 relative (or 5e-6), tensors 1e-4 relative + 1e-4 max(1, max |ref|), gradient norms
    2e-3 relative + 1e-7, full gradients 2e-3 relative L2, parameter |.| sums 2e-6 relative.  acc_map per frame EXACTLY (the
    generator made every cell's top-two gap of map_rec exceed 1e-4)."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    oconf, model = _model(g)
    I, C = oconf.iwae_samples, model.probe_model.map_channels
    assert I == (2 if name.endswith('iwae') else 1) and float(g['min_map_rec_gap']) > 1e-4 and float(g['min_edge_distance']) > 1e-5
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    state = model.init_state(oconf.batch_size * I)
    for s in range(steps):
        pre = f's{s}_'
        obs, noise = _obs(g, pre, oconf, C)
        seen = g[pre + 'in_map_seen_mask']
        assert (seen.reshape(-1, seen.shape[-1] ** 2).sum(-1) == 0).sum() == 1, 'one frame without a seen cell'
        losses, state, metrics, tensors, _ = model.training_step(obs, state, noise=noise)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        for opt in opts:
            opt.step()
        assert np.array_equal(model.last_extras['post_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_post']), (s, 'posterior indices')
        assert np.array_equal(model.last_extras['act_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_act']), (s, 'action indices')
        for i, l in enumerate(losses):
            ref = g[pre + 'losses'][i]
            print(f'step {s} loss {i}: {float(l.detach()):.8g} reference {ref:.8g} rel {_rel(l.detach(), ref):.2e}')
            assert _rel(l.detach(), ref) < 2e-5 or abs(float(l) - ref) < 2e-6, (s, i, float(l), ref)
        allm = {**metrics, **gm}
        assert {'loss_map', 'acc_map', 'acc_map_seen', 'grad_norm_probe'} <= set(allm)
        for k in allm:
            ref = float(g[pre + 'metric_' + k])
            if k in ('loss_map', 'acc_map', 'acc_map_seen', 'grad_norm_probe'):
                print(f'step {s} {k}: {float(allm[k]):.8g} reference {ref:.8g} rel {_rel(allm[k], ref):.2e}')
            assert _rel(allm[k], ref) < 1e-4 or abs(float(allm[k]) - ref) < 5e-6, (s, k, float(allm[k]), ref)
        assert float(metrics['loss_map']) == float(losses[1])
        for k in ('map_rec', 'loss_map', 'acc_map'):
            ref = torch.from_numpy(g[pre + 'tensor_' + k])
            assert tensors[k].shape == ref.shape
            _close_rt(tensors[k], ref, 1e-4, 1e-4 * max(1.0, float(ref.abs().max())), f'step {s} {k}')
        assert torch.equal(tensors['acc_map'].cpu(), torch.from_numpy(g[pre + 'tensor_acc_map'])), f'step {s}: acc_map per frame'
        names = [str(n) for n in g[pre + 'probe_grad_names']]
        assert names == [k for k in grads if k.startswith('probe_model.')]
        for n, ref in zip(names, g[pre + 'probe_grad_norms']):
            got = float(grads[n].double().norm())
            assert abs(got - ref) <= 2e-3 * ref + 1e-7, (s, n, got, ref)
        full = [k for k in g.files if k.startswith(pre + 'grad_probe_model.')]
        assert len(full) == 2
        for k in full:
            e = _rel_l2(grads[k[len(pre + 'grad_'):]], torch.from_numpy(g[k]))
            print(f'step {s} full gradient {k[len(pre + "grad_"):]}: relative L2 error {e:.3e}')
            assert e < 2e-3, (s, k, e)
        sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
        np.testing.assert_allclose(sums, g[pre + 'param_abs_sums'], rtol=2e-6)
    names, buf, idx = model.packed_metrics()
    vals = dict(zip(names, (buf.tolist()[i] for i in idx)))
    for k in ('loss_map', 'acc_map', 'acc_map_seen'):
        assert vals[k] == float(metrics[k]), k


def _one_step(model, g, oconf, C, backward=True):
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    obs, noise = _obs(g, 's0_', oconf, C)
    if model.conf.probe_model == 'none':
        obs = {k: v for k, v in obs.items() if not k.startswith('map')}
    losses, _, metrics, tensors, _ = model.training_step(obs, model.init_state(oconf.batch_size * oconf.iwae_samples), noise=noise)
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
    grads = [o.flat_grad.clone() for o in opts]
    for opt in opts:
        opt.step()
    torch.cuda.synchronize()
    return losses, metrics, grads, [o.flat_param.clone() for o in opts], obs, noise


@pytest.mark.parametrize('name', ['tiny_map_probe', 'tiny_map_probe_iwae'])
def test_bit_identity_and_independence(hip, name):
    """(1) Parameters after backward / grad_clip / step are bit-identical for overlap_backward True and False.  (2) The probe reads
    detached features only: the world-model, actor and critic losses and gradients are bit-identical to a probe_model='none' run of
    the same step, and that run's three map slots of the metric buffer stay zero.  (3) A second loss_probe.backward() on the
    released step raises.  (4) The data-parallel shard weight scales the probe gradients: grad_weight = 0.5 halves them exactly."""
    from pydreamer_amd.models import METRIC_SLOTS
    g = np.load(os.path.join(GOLD, name + '.npz'))
    runs = []
    for overlap in (True, False):
        oconf, model = _model(g)
        assert model.overlap_backward
        model.overlap_backward = overlap
        runs.append(_one_step(model, g, oconf, model.probe_model.map_channels))
    C = model.probe_model.map_channels
    (la, ma, ga, pa, _, _), (lb, mb, gb, pb, _, _) = runs
    assert [float(x) for x in la] == [float(x) for x in lb]
    for a, b in zip(ga + pa, gb + pb):
        assert torch.equal(a, b), 'overlap_backward changes gradients or parameters'
    assert float(ga[1].abs().sum()) > 0 and len(pa) == 4
    with pytest.raises(RuntimeError):
        runs[0][0][1].backward()
    oconf, none = _model(g, probe_model='none')
    ln, mn, gn, pn, _, _ = _one_step(none, g, oconf, C)
    for i in (0, 2, 3):
        assert float(ln[i]) == float(la[i]), (i, float(ln[i]), float(la[i]))
        assert torch.equal(gn[i], ga[i]) and torch.equal(pn[i], pa[i]), f'group {i} depends on the probe'
    for k in ('loss_map', 'acc_map', 'acc_map_seen'):
        assert float(none.metric_buffer[METRIC_SLOTS[k]]) == 0.0 and k not in mn
    oconf, half = _model(g)
    half.probe_model.grad_weight = 0.5
    lh, _, gh, _, _, _ = _one_step(half, g, oconf, C)
    # (grad_clip's coefficient is 1 here: the norm is far below the clip)
    assert float(lh[1]) == float(la[1]) and torch.equal(gh[1] * 2, ga[1]), 'grad_weight = 0.5 must halve the probe gradients exactly'


def test_inputs_are_checked_and_evaluation_runs_without_grad(hip):
    g = np.load(os.path.join(GOLD, 'tiny_map_probe.npz'))
    oconf, model = _model(g)
    C = model.probe_model.map_channels
    obs, noise = _obs(g, 's0_', oconf, C)
    state = model.init_state(oconf.batch_size)
    with torch.no_grad():
        losses, _, metrics, tensors, _ = model.training_step(obs, state, noise=noise)
        assert not losses[1].requires_grad and _rel(losses[1], g['s0_losses'][1]) < 2e-5
        assert _rel(metrics['acc_map_seen'], float(g['s0_metric_acc_map_seen'])) < 1e-4
        no_mask = {k: v for k, v in obs.items() if k != 'map_seen_mask'}
        _, _, m2, _, _ = model.training_step(no_mask, state, noise=noise)
        assert 'acc_map_seen' not in m2 and float(m2['acc_map']) == float(metrics['acc_map'])
        for gone in ('map', 'map_coord'):
            with pytest.raises(ValueError):
                model.training_step({k: v for k, v in obs.items() if k != gone}, state, noise=noise)
        for k, bad in (('map_coord', obs['map_coord'][..., :3]), ('map', obs['map'][:, :, :-1]), ('map', obs['map'][..., :-1]),
                       ('map_seen_mask', obs['map_seen_mask'][:, :, :-1])):
            with pytest.raises(ValueError) as e:
                model.training_step(dict(obs, **{k: bad.contiguous()}), state, noise=noise)
            assert 'training_step input shapes (got, expected)' in str(e.value) and k in str(e.value)
