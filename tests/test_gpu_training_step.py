"""-m gpu: the HIP training path (through the C-ABI) against the CPU oracle and the reference-generated goldens.

Bars (fp32, stated per assertion): sampled indices bit-exact (same uniforms, inverse-CDF rule); losses / metrics
within 2e-5 relative (loss_model additionally within 1e-3 absolute, the north-star bar); per-parameter gradients
within 2e-3 relative L2 error; parameters after clip + AdamW within 1e-5 absolute (lr 3e-4 step).
"""
import ast
import contextlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_reference as CR
from oracle import dreamer_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/rssm_sequence_case.py

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def _hip_conf(oconf):
    from pydreamer_amd import config
    keys = {k: getattr(oconf, k) for k in vars(oconf)}
    return config.load_config('defaults', 'atari', **keys)


def _build(oconf, params):
    from pydreamer_amd.models import Dreamer
    model = Dreamer(_hip_conf(oconf))
    model.load_state_dict(params, strict=True)
    return model.to(DEV)


def _to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-12)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _close(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e})'


# ------------------------------------------------------------------------------------------- operators
def test_mlp_head_fwd_bwd(hip):
    from pydreamer_amd.models import MLP
    rows, in_dim, out_dim = 300, 136, 6
    torch.manual_seed(0)
    m = MLP(in_dim, out_dim, 400, 4).to(DEV)
    x = torch.randn(rows, in_dim, device=DEV)
    dout = torch.randn(rows, out_dim, device=DEV)
    ws = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
    out, acts = m.fwd(x, in_dim, rows, ws)
    dx = torch.zeros(rows, in_dim, device=DEV)
    grads, _, _ = m.bwd(x, in_dim, rows, acts, dout, ws, dx=dx, lddx=in_dim, dx_accum=False)
    p = {f'h.{k}': v.detach().double().cpu().requires_grad_(True) for k, v in m.model.state_dict().items()}
    xr = x.double().cpu().requires_grad_(True)
    ref = O.mlp(p, 'h', xr, 4)
    _close(out, ref, 1e-4, 1e-5, 'mlp fwd')
    ref.backward(dout.double().cpu())
    _close(dx, xr.grad, 1e-3, 1e-5, 'mlp dx')
    for (name, _), g in zip(m.named_parameters(), grads):
        key = 'h.' + name.replace('model.', '', 1)
        assert _rel_l2(g, p[key].grad) < 1e-4, name


@pytest.mark.parametrize('rows,in_dim,out_dim', [(16400, 136, 6), (16384, 1624, 1), (20000, 400, 18)])
def test_mlp_head_panel_fwd_bwd(hip, rows, in_dim, out_dim):
    """rows >= 16384: every Linear -> LayerNorm -> ELU is one row-panel launch (csrc/panel.hip), the output layer rides in
    the last one's epilogue, and backward fuses dgrad + LayerNorm/ELU backward + the bias / gamma / beta column sums.
    Ragged last panel (16400 = 256*64 + 16), K = 1 / 6 / 18 data-gradient products (unaligned scalar-load path).
    Same tolerances as the GEMM + LayerNorm path's test above; also: the acts-free forward gives identical outputs."""
    from pydreamer_amd.models import MLP
    torch.manual_seed(1)
    m = MLP(in_dim, out_dim, 400, 4).to(DEV)
    with torch.no_grad():                      # non-trivial LayerNorm parameters
        for i in range(4):
            m.model[3 * i + 1].weight.uniform_(0.5, 1.5)
            m.model[3 * i + 1].bias.uniform_(-0.5, 0.5)
    x = torch.randn(rows, in_dim, device=DEV)
    dout = torch.randn(rows, out_dim, device=DEV) / rows
    ws = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    out, acts = m.fwd(x, in_dim, rows, ws)
    out2, none = m.fwd(x, in_dim, rows, ws, save_acts=False)
    assert none is None and torch.equal(out, out2)
    dx = torch.zeros(rows, in_dim, device=DEV)
    grads, _, _ = m.bwd(x, in_dim, rows, acts, dout, ws, dx=dx, lddx=in_dim, dx_accum=False)
    p = {f'h.{k}': v.detach().double().cpu().requires_grad_(True) for k, v in m.model.state_dict().items()}
    xr = x.double().cpu().requires_grad_(True)
    ref = O.mlp(p, 'h', xr, 4)
    _close(out, ref.reshape(out.shape), 1e-4, 1e-5, 'panel mlp fwd')
    ref.backward(dout.double().cpu().reshape(ref.shape))
    assert _rel_l2(dx, xr.grad) < 1e-4, 'panel mlp dx'
    for (name, _), g in zip(m.named_parameters(), grads):
        key = 'h.' + name.replace('model.', '', 1)
        assert _rel_l2(g, p[key].grad) < 1e-4, name


@pytest.mark.parametrize('rows,dense,S,C,out_dim', [(16400, 72, 8, 8, 6), (20000, 600, 32, 32, 1), (2500, 600, 32, 32, 18),
                                                    (1100, 64, 8, 8, 6)])
def test_mlp_head_sparse_trailing_columns(hip, rows, dense, S, C, out_dim):
    """dm_mlp_head_fwd_sparse (layer 0 = dense columns on the matrix pipe + the one-hot latent columns as a sum of weight
    rows) equals dm_mlp_head_fwd on feature rows [h | one-hot z] - output, saved pre-activations and statistics, so the
    unchanged dm_mlp_head_bwd gives the same gradients - and stays EXACT for arbitrary (dense, scaled, all-zero) trailing
    columns; fp64 reference; bf16 operands too.  Rows >= 16 384: the row-panel kernels; 256 <= rows < 16 384: the whole-MLP
    kernel (weights packed for the dense columns only, the addend joins the layer-0 pre-activation before the LayerNorm)."""
    from pydreamer_amd.models import MLP
    torch.manual_seed(11)
    Z = S * C
    in_dim = dense + Z
    m = MLP(in_dim, out_dim, 400, 4).to(DEV)
    ws = torch.empty(768 << 20, dtype=torch.uint8, device=DEV)
    idx = torch.randint(0, C, (rows, S), device=DEV)
    z = F.one_hot(idx, C).float().reshape(rows, Z)
    x = torch.cat((torch.randn(rows, dense, device=DEV), z), -1).contiguous()
    out_d, acts_d = m.fwd(x, in_dim, rows, ws, acts=torch.zeros(m.acts_floats(rows), device=DEV))
    out_s, acts_s = m.fwd(x, in_dim, rows, ws, acts=torch.zeros(m.acts_floats(rows), device=DEV), sparse_cols=Z)
    sd = {k: v.detach().double().cpu() for k, v in m.model.state_dict().items()}
    h = x.double().cpu()
    for i in range(4):
        h = F.elu(F.layer_norm(h @ sd[f'{3 * i}.weight'].t() + sd[f'{3 * i}.bias'], (400,), sd[f'{3 * i + 1}.weight'],
                               sd[f'{3 * i + 1}.bias'], 1e-3))
    ref = (h @ sd['12.weight'].t() + sd['12.bias']).reshape(out_s.shape)
    e_s, e_d = float((out_s.double().cpu() - ref).abs().max()), float((out_d.double().cpu() - ref).abs().max())
    assert e_s < 2e-5 * max(1.0, float(ref.abs().max())) and e_s < 4 * e_d + 1e-6, (e_s, e_d)
    assert _rel_l2(acts_s, acts_d) < 2e-6
    dout = torch.randn(rows, out_dim, device=DEV) / rows
    g_s = [g.clone() for g in m.bwd(x, in_dim, rows, acts_s, dout, ws)[0]]
    g_d = [g.clone() for g in m.bwd(x, in_dim, rows, acts_d, dout, ws)[0]]
    for a_, b_ in zip(g_s, g_d):
        assert _rel_l2(a_, b_) < 1e-5
    # not one-hot at all: scaled, dense and empty trailing columns - the sparse-row product is exact for any input
    x2 = x.clone()
    x2[: rows // 3, dense:] = torch.randn(rows // 3, Z, device=DEV)
    x2[rows // 3: rows // 2, dense:] *= 2.5
    x2[rows // 2: rows // 2 + 7, dense:] = 0
    o_d, _ = m.fwd(x2, in_dim, rows, ws, save_acts=False)
    o_s, _ = m.fwd(x2, in_dim, rows, ws, save_acts=False, sparse_cols=Z)
    assert _rel_l2(o_s, o_d) < 2e-6 and float((o_s - o_d).abs().max()) < 2e-5 * max(1.0, float(o_d.abs().max()))
    # bf16 operands (conf.amp) keep the full product (the gather does not pay there): identical results
    m.precision = 1
    o16_d, _ = m.fwd(x, in_dim, rows, ws, save_acts=False)
    o16_s, _ = m.fwd(x, in_dim, rows, ws, save_acts=False, sparse_cols=Z)
    assert torch.equal(o16_s, o16_d)


@pytest.mark.parametrize('rows,in_dim,out_dim', [(16400, 136, 6), (20000, 1624, 1)])
def test_mlp_head_panel_bf16_operands(hip, rows, in_dim, out_dim):
    """dm_mlp_params.precision = 1 (conf.amp) on the row-panel path: operands of every hidden-layer product rounded to bf16
    (RNE), fp32 accumulation, fp32 LayerNorm / ELU / output layer.  Forward against exactly that arithmetic in fp64
    (only the summation order differs: fp32-class tolerance); gradients against the fp32 path's at a bf16-class bound
    (2^-8 operand rounding), and deterministic."""
    from pydreamer_amd.models import MLP
    torch.manual_seed(5)
    m = MLP(in_dim, out_dim, 400, 4).to(DEV)
    with torch.no_grad():
        for i in range(4):
            m.model[3 * i + 1].weight.uniform_(0.5, 1.5)
            m.model[3 * i + 1].bias.uniform_(-0.5, 0.5)
    x = torch.randn(rows, in_dim, device=DEV)
    dout = torch.randn(rows, out_dim, device=DEV) / rows
    ws = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    dx32 = torch.zeros(rows, in_dim, device=DEV)
    out32, acts32 = m.fwd(x, in_dim, rows, ws)
    g32 = [g.clone() for g in m.bwd(x, in_dim, rows, acts32, dout, ws, dx=dx32, lddx=in_dim)[0]]
    m.precision = 1
    out, acts = m.fwd(x, in_dim, rows, ws)
    dx = torch.zeros(rows, in_dim, device=DEV)
    g16 = [g.clone() for g in m.bwd(x, in_dim, rows, acts, dout, ws, dx=dx, lddx=in_dim)[0]]
    out_b, acts_b = m.fwd(x, in_dim, rows, ws)
    assert torch.equal(out, out_b)
    # forward emulation: bf16-rounded operands, fp64 accumulation, everything else fp64
    h = x.double().cpu()
    sd = {k: v.detach().double().cpu() for k, v in m.model.state_dict().items()}
    for i in range(4):
        pre = h.float().bfloat16().double() @ sd[f'{3 * i}.weight'].float().bfloat16().double().t() + sd[f'{3 * i}.bias']
        pre = F.layer_norm(pre, (400,), sd[f'{3 * i + 1}.weight'], sd[f'{3 * i + 1}.bias'], 1e-3)
        h = F.elu(pre)
    ref = h @ sd['12.weight'].t() + sd['12.bias']                 # the fused output layer stays fp32 (a row reduction)
    # an fp32-vs-fp64 difference in a hidden activation can flip its bf16 rounding (2^-8 relative on that element), so the
    # bound is bf16-class per element - but the result must sit much closer to the bf16 arithmetic than to the fp32 one
    err = (out.double().cpu() - ref.reshape(out.shape)).abs()
    gap = (out32.double().cpu() - ref.reshape(out.shape)).abs()
    assert float(err.max()) < 5e-3 and float(err.mean()) < 0.2 * float(gap.mean()), (float(err.max()), float(err.mean()), float(gap.mean()))
    assert _rel_l2(dx, dx32) < 2e-2
    for a, b in zip(g16, g32):
        assert _rel_l2(a, b) < 2e-2


@pytest.mark.parametrize('rows,in_dim,out_dim,layers', [(2500, 1624, 18, 4), (350, 1624, 1, 4), (17, 136, 6, 2), (1, 400, 32, 1)])
def test_mlp_head_chain_fwd_bwd(hip, rows, in_dim, out_dim, layers):
    """rows below the panel threshold: the WHOLE forward ([Linear -> LayerNorm -> ELU] x L -> Linear) is one launch
    (csrc/mlp_chain.hip: 16-row blocks, activations in LDS between layers, K split over the 4 waves).  Ragged last block,
    a K that is not a multiple of 16 (1624 = 101.5 groups), 1..4 layers, a single row.  The saved activations must be
    what the per-layer backward expects (gradients checked through dm_mlp_head_bwd); the acts-free call gives identical
    outputs; dm_mlp_chain_min_rows is the A/B switch back to GEMM + LayerNorm launches."""
    from pydreamer_amd.models import MLP
    prev = hip.lib().dm_mlp_chain_min_rows(1)            # the production threshold is 256 rows
    try:
        _chain_case(rows, in_dim, out_dim, layers)
    finally:
        hip.lib().dm_mlp_chain_min_rows(prev)


def _chain_case(rows, in_dim, out_dim, layers):
    from pydreamer_amd.models import MLP
    torch.manual_seed(3)
    m = MLP(in_dim, out_dim, 400, layers).to(DEV)
    with torch.no_grad():
        for i in range(layers):
            m.model[3 * i + 1].weight.uniform_(0.5, 1.5)
            m.model[3 * i + 1].bias.uniform_(-0.5, 0.5)
    ld = in_dim + 8                                    # a strided input (feature-matrix rows)
    xs = torch.randn(rows, ld, device=DEV)
    x = xs[:, :in_dim]
    dout = torch.randn(rows, out_dim, device=DEV) / rows
    ws = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
    out, acts = m.fwd(xs, ld, rows, ws)
    out2, none = m.fwd(xs, ld, rows, ws, save_acts=False)
    assert none is None and torch.equal(out, out2)
    dx = torch.zeros(rows, in_dim, device=DEV)
    grads, _, _ = m.bwd(xs, ld, rows, acts, dout, ws, dx=dx, lddx=in_dim, dx_accum=False)
    p = {f'h.{k}': v.detach().double().cpu().requires_grad_(True) for k, v in m.model.state_dict().items()}
    xr = x.double().cpu().requires_grad_(True)
    ref = O.mlp(p, 'h', xr, layers)
    _close(out, ref.reshape(out.shape), 1e-4, 1e-5, 'chain mlp fwd')
    ref.backward(dout.double().cpu().reshape(ref.shape))
    assert _rel_l2(dx, xr.grad) < 1e-4, 'chain mlp dx'
    for (name, _), g in zip(m.named_parameters(), grads):
        key = 'h.' + name.replace('model.', '', 1)
        assert _rel_l2(g, p[key].grad) < 1e-4, name


def test_mlp_head_chain_bf16_operands(hip):
    """precision = 1 on the whole-MLP forward kernel: the hidden-layer products run on bf16 MFMA with fp32 accumulation.
    Same bars as the row-panel bf16 test (bf16-class per element, far closer to the bf16 arithmetic than to fp32)."""
    from pydreamer_amd.models import MLP
    rows, in_dim, out_dim = 2500, 1624, 18
    torch.manual_seed(6)
    m = MLP(in_dim, out_dim, 400, 4).to(DEV)
    x = torch.randn(rows, in_dim, device=DEV)
    ws = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
    out32, _ = m.fwd(x, in_dim, rows, ws)
    m.precision = 1
    out, acts = m.fwd(x, in_dim, rows, ws)
    out_b, _ = m.fwd(x, in_dim, rows, ws, save_acts=False)
    assert torch.equal(out, out_b)
    h = x.double().cpu()
    sd = {k: v.detach().double().cpu() for k, v in m.model.state_dict().items()}
    for i in range(4):
        pre = h.float().bfloat16().double() @ sd[f'{3 * i}.weight'].float().bfloat16().double().t() + sd[f'{3 * i}.bias']
        h = F.elu(F.layer_norm(pre, (400,), sd[f'{3 * i + 1}.weight'], sd[f'{3 * i + 1}.bias'], 1e-3))
    ref = h @ sd['12.weight'].t() + sd['12.bias']
    err = (out.double().cpu() - ref).abs()
    gap = (out32.double().cpu() - ref).abs()
    assert float(err.max()) < 5e-3 and float(err.mean()) < 0.2 * float(gap.mean()), (float(err.max()), float(err.mean()), float(gap.mean()))


@pytest.mark.parametrize('depth,T,B', [(8, 2, 3), (48, 2, 2)])
def test_conv_encoder_fwd_bwd(hip, depth, T, B):
    """dm_conv_encoder_fwd / _bwd through the C-ABI against the fp64 oracle (encoders.py:80-96), FULL tensors: the embedding and
    every weight / bias gradient.  depth 48 is the shipped cnn_depth (defaults.yaml:78): the direct layer-1 kernels
    enc_l1_fwd_kernel<48> / enc_l1_wgrad_kernel are templated on it and are not reached at depth 8."""
    import ctypes
    from pydreamer_amd import hip as H
    oconf = O.tiny_conf(cnn_depth=depth)
    params = O.make_params(oconf)
    model = _build(oconf, params)
    image = (torch.rand(T, B, 3, 64, 64, generator=torch.Generator().manual_seed(1)) - 0.5).to(DEV)
    shp = model.wm.shape(T, B, 1)
    ws = model.wm.workspace(shp, torch.device(DEV, 0))
    enc = model.wm.encoder.encoder_image
    N, E = T * B, enc.out_dim
    enc_p = H.conv_struct([m.weight for m in enc.convs()], [m.bias for m in enc.convs()])
    acts = torch.empty(int(H.lib().dm_conv_encoder_acts_floats(ctypes.byref(shp))), device=DEV)
    embed = torch.empty(N, E, device=DEV)
    H.call('dm_conv_encoder_fwd', ctypes.byref(shp), H.fptr(image), ctypes.byref(enc_p), H.fptr(acts), H.fptr(embed),
           H.ptr(ws), ws.numel(), H.stream())
    p = {k: v.double().requires_grad_(True) for k, v in params.items() if 'encoder' in k}
    ref = O.conv_encoder(p, image.double().cpu())
    _close(embed.view(T, B, E), ref, 1e-4, 1e-5, 'encoder fwd')
    dembed = torch.randn(N, E, generator=torch.Generator().manual_seed(2)).to(DEV)
    ref.backward(dembed.view(T, B, E).double().cpu())
    grads = [torch.empty_like(m.weight) for m in enc.convs()], [torch.empty_like(m.bias) for m in enc.convs()]
    enc_g = H.conv_struct(grads[0], grads[1], cls=H.dm_conv_grads)
    H.call('dm_conv_encoder_bwd', ctypes.byref(shp), H.fptr(image), ctypes.byref(enc_p), H.fptr(acts), H.fptr(dembed),
           ctypes.byref(enc_g), H.ptr(ws), ws.numel(), H.stream())
    for i in range(4):
        assert _rel_l2(grads[0][i], p[f'wm.encoder.encoder_image.model.{2 * i}.weight'].grad) < 2e-4, f'conv{i} dW'
        assert _rel_l2(grads[1][i], p[f'wm.encoder.encoder_image.model.{2 * i}.bias'].grad) < 2e-4, f'conv{i} db'
    # ... and element by element: max |got - ref64| / rms(ref64) within 10x what the oracle's own fp32 arithmetic misses fp64 by
    # (oracle/conv_reference.py; tests/test_gpu_conv_stack.py does the same at production frame counts)
    frames, dcpu = image.cpu().reshape(N, 3, 64, 64), dembed.cpu()
    r64, r32 = (CR.encoder_reference(params, frames, dcpu, dtype=dt) for dt in (torch.float64, torch.float32))
    CR.check_tensor('encoder embed', embed.cpu(), r64['embed'], r32['embed'], ('frame', 'feature(c,y,x)'))
    for i in range(4):
        CR.check_tensor(f'encoder dW{i}', grads[0][i].cpu(), r64[f'dW{i}'], r32[f'dW{i}'], ('out', 'in', 'ky', 'kx'))
        CR.check_tensor(f'encoder db{i}', grads[1][i].cpu(), r64[f'db{i}'], r32[f'db{i}'], ('out',))


@pytest.mark.parametrize('depth,l4_direct', [(8, 1), (8, 0), (16, 1), (48, 1), (48, 0), (64, 1)])
def test_conv_decoder_mse_fwd_bwd(hip, depth, l4_direct):
    """dm_conv_decoder_mse_fwd / _bwd through the C-ABI against the fp64 oracle (decoders.py:144-167), FULL tensors: the decoded
    image, the per-frame loss, the feature gradient and every weight / bias gradient.  depth 48 (the shipped cnn_depth)
    reaches dec_l4_fwd_kernel<48>, which depth 8 does not.  l4_direct: the image layer's backward as the two direct MFMA
    kernels (dec_l4_dgrad_kernel / dec_l4_wgrad_kernel; depth 8 = a partly filled 16-channel block, 64 = four blocks) or as
    gather-form products through the tile kernels."""
    import ctypes
    from pydreamer_amd import hip as H
    H.lib().dm_dec_l4_bwd_direct_enable(l4_direct)
    try:
        _conv_decoder_mse_fwd_bwd(depth)
    finally:
        H.lib().dm_dec_l4_bwd_direct_enable(1)


def _conv_decoder_mse_fwd_bwd(depth):
    import ctypes
    from pydreamer_amd import hip as H
    oconf = O.tiny_conf(cnn_depth=depth)
    params = O.make_params(oconf)
    model = _build(oconf, params)
    T, B = 2, 2
    N, F_ = T * B, model.wm.features_dim
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(N, F_, generator=g).to(DEV)
    target = (torch.rand(N, 3, 64, 64, generator=g) - 0.5).to(DEV)
    shp = model.wm.shape(T, B, 1)
    ws = model.wm.workspace(shp, torch.device(DEV, 0))
    dl = model.wm.decoder.image.layers()
    dec_p = H.conv_struct([m.weight for m in dl], [m.bias for m in dl])
    acts = torch.empty(int(H.lib().dm_conv_decoder_acts_floats(ctypes.byref(shp))), device=DEV)
    loss = torch.empty(N, device=DEV)
    rec = torch.empty(N, 3, 64, 64, device=DEV)
    H.call('dm_conv_decoder_mse_fwd', ctypes.byref(shp), H.fptr(feat), F_, H.fptr(target), ctypes.byref(dec_p),
           H.fptr(acts), H.fptr(loss), H.fptr(rec), H.ptr(ws), ws.numel(), H.stream())
    p = {k: v.double().requires_grad_(True) for k, v in params.items() if 'decoder.image' in k}
    fr = feat.double().cpu().requires_grad_(True)
    dec = O.conv_decoder(p, fr)
    lref = 0.5 * torch.square(dec - target.double().cpu()).sum(dim=[-1, -2, -3])
    _close(rec, dec, 1e-4, 2e-5, 'decoder image_rec')
    _close(loss, lref, 1e-5, 1e-4, 'decoder loss')
    scale = 1.0 / N
    (lref.sum() * scale).backward()
    gw, gb = [torch.empty_like(m.weight) for m in dl], [torch.empty_like(m.bias) for m in dl]
    dec_g = H.conv_struct(gw, gb, cls=H.dm_conv_grads)
    dfeat = torch.ones(N, F_, device=DEV)
    H.call('dm_conv_decoder_mse_bwd', ctypes.byref(shp), H.fptr(feat), F_, H.fptr(target), ctypes.byref(dec_p),
           H.fptr(acts), scale, ctypes.byref(dec_g), H.fptr(dfeat), F_, H.ptr(ws), ws.numel(), H.stream())
    assert _rel_l2(dfeat - 1.0, fr.grad) < 2e-4, 'decoder dfeat (accumulated onto ones)'
    for i, idx in enumerate((0, 2, 4, 6, 8)):
        assert _rel_l2(gw[i], p[f'wm.decoder.image.model.{idx}.weight'].grad) < 2e-4, f'dec layer {i} dW'
        assert _rel_l2(gb[i], p[f'wm.decoder.image.model.{idx}.bias'].grad) < 2e-4, f'dec layer {i} db'
    # ... and element by element (see test_conv_encoder_fwd_bwd).  dfeat was accumulated onto ones: the reference is 1 + gradient,
    # summed in fp64 and - for the bar - in fp32, so the rounding of that sum is part of both
    r64, r32 = (CR.decoder_reference(params, feat.cpu(), target.cpu(), scale, dtype=dt) for dt in (torch.float64, torch.float32))
    CR.check_tensor('decoder image_rec', rec.cpu(), r64['image_rec'], r32['image_rec'], ('frame', 'channel', 'y', 'x'))
    CR.check_tensor('decoder loss_image', loss.cpu(), r64['loss_image'], r32['loss_image'], ('frame',))
    CR.check_tensor('decoder dfeat + 1', dfeat.cpu(), 1.0 + r64['dfeat'], 1.0 + r32['dfeat'], ('frame', 'feature'))
    for i in range(5):
        axes = ('out', 'in') if i == 0 else ('in', 'out', 'ky', 'kx')
        CR.check_tensor(f'decoder dW{i}', gw[i].cpu(), r64[f'dW{i}'], r32[f'dW{i}'], axes)
        CR.check_tensor(f'decoder db{i}', gb[i].cpu(), r64[f'db{i}'], r32[f'db{i}'], ('out',))


def _conv_stack_bf16(model, T, B, twins, seed=5, flip_before_backward=False):
    """Encoder fwd+bwd and decoder fwd+bwd through the C-ABI with DM_FLAG_BF16, the bf16-storage operand path on / off."""
    import ctypes
    from pydreamer_amd import hip as H
    H.lib().dm_bf16_twins_enable(1 if twins else 0)
    try:
        g = torch.Generator().manual_seed(seed)
        shp = model.wm.shape(T, B, 1)
        shp.flags |= H.DM_FLAG_BF16
        ws = torch.empty(H.workspace_bytes(shp), dtype=torch.uint8, device=DEV)
        enc = model.wm.encoder.encoder_image
        N, E, F_ = T * B, enc.out_dim, model.wm.features_dim
        image = (torch.rand(T, B, 3, 64, 64, generator=g) - 0.5).to(DEV)
        feat = torch.randn(N, F_, generator=g).to(DEV)
        dembed = torch.randn(N, E, generator=g).to(DEV)
        enc_p = H.conv_struct([m.weight for m in enc.convs()], [m.bias for m in enc.convs()])
        acts = torch.empty(int(H.lib().dm_conv_encoder_acts_floats(ctypes.byref(shp))), device=DEV)
        embed = torch.empty(N, E, device=DEV)
        H.call('dm_conv_encoder_fwd', ctypes.byref(shp), H.fptr(image), ctypes.byref(enc_p), H.fptr(acts), H.fptr(embed),
               H.ptr(ws), ws.numel(), H.stream())
        eg = [torch.empty_like(m.weight) for m in enc.convs()], [torch.empty_like(m.bias) for m in enc.convs()]
        enc_g = H.conv_struct(eg[0], eg[1], cls=H.dm_conv_grads)
        if flip_before_backward:
            acts[int(H.lib().dm_conv_encoder_acts_floats(ctypes.byref(model.wm.shape(T, B, 1)))):].fill_(float('nan'))   # the (unwritten) twin region
            H.lib().dm_bf16_twins_enable(0 if twins else 1)
        H.call('dm_conv_encoder_bwd', ctypes.byref(shp), H.fptr(image), ctypes.byref(enc_p), H.fptr(acts), H.fptr(dembed),
               ctypes.byref(enc_g), H.ptr(ws), ws.numel(), H.stream())
        H.lib().dm_bf16_twins_enable(1 if twins else 0)
        dl = model.wm.decoder.image.layers()
        dec_p = H.conv_struct([m.weight for m in dl], [m.bias for m in dl])
        dacts = torch.empty(int(H.lib().dm_conv_decoder_acts_floats(ctypes.byref(shp))), device=DEV)
        loss = torch.empty(N, device=DEV)
        rec = torch.empty(N, 3, 64, 64, device=DEV)
        target = image.reshape(N, 3, 64, 64).contiguous()
        H.call('dm_conv_decoder_mse_fwd', ctypes.byref(shp), H.fptr(feat), F_, H.fptr(target), ctypes.byref(dec_p),
               H.fptr(dacts), H.fptr(loss), H.fptr(rec), H.ptr(ws), ws.numel(), H.stream())
        dg = [torch.empty_like(m.weight) for m in dl], [torch.empty_like(m.bias) for m in dl]
        dec_g = H.conv_struct(dg[0], dg[1], cls=H.dm_conv_grads)
        if flip_before_backward:
            dacts[int(H.lib().dm_conv_decoder_acts_floats(ctypes.byref(model.wm.shape(T, B, 1)))):].fill_(float('nan'))
            H.lib().dm_bf16_twins_enable(0 if twins else 1)
        dfeat = torch.zeros(N, F_, device=DEV)
        H.call('dm_conv_decoder_mse_bwd', ctypes.byref(shp), H.fptr(feat), F_, H.fptr(target), ctypes.byref(dec_p),
               H.fptr(dacts), 1.0 / N, ctypes.byref(dec_g), H.fptr(dfeat), F_, H.ptr(ws), ws.numel(), H.stream())
        torch.cuda.synchronize()
        out = dict(embed=embed, loss=loss, rec=rec, dfeat=dfeat)
        for i in range(4):
            out[f'enc_dw{i}'], out[f'enc_db{i}'] = eg[0][i], eg[1][i]
        for i in range(5):
            out[f'dec_dw{i}'], out[f'dec_db{i}'] = dg[0][i], dg[1][i]
        return {k: v.double().cpu() for k, v in out.items()}
    finally:
        H.lib().dm_bf16_twins_enable(1)


@pytest.mark.parametrize('depth,T,B', [(8, 2, 3), (48, 2, 2), (16, 3, 5), (48, 1, 513), (48, 50, 50), (64, 1, 3)])
def test_conv_bf16_storage_twins_match_fp32_storage(hip, depth, T, B):
    """conf.amp convolution stack with operands STORED as bf16 (twins written by the producing kernels, gemm_h_kernel) against
    the same bf16 products fed from fp32 storage (rounded on the way into LDS): the operand values are identical (RNE of
    the same fp32 numbers), so results differ by fp32 summation order only - every output and gradient within 2e-5 relative."""
    oconf = O.tiny_conf(cnn_depth=depth)
    model = _build(oconf, O.make_params(oconf))
    a = _conv_stack_bf16(model, T, B, twins=True)
    b = _conv_stack_bf16(model, T, B, twins=False)
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        assert _rel_l2(a[k], b[k]) < 2e-5, (k, _rel_l2(a[k], b[k]))
    # the switch flipped BETWEEN forward and backward: the backward must not trust twins that were never written
    c = _conv_stack_bf16(model, T, B, twins=False, flip_before_backward=True)
    for k in a:
        assert _rel_l2(c[k], b[k]) < 2e-5, (k, 'switch flipped between forward and backward')


def test_dream_rollout_bf16_storage_twins_match_fp32_storage(hip):
    """conf.amp imagination rollout at the Atari-literal cell width (deter 600, hidden 1000, stoch 32x32), 300 rows: the cell's
    four products fed from bf16 twins (per-call weight copies, za and the h columns of the feature buffer written by the
    producing kernels) against the same bf16 products fed from fp32 storage - same operand values, so the sampled actions are
    identical and the features agree to fp32 summation order."""
    from pydreamer_amd import config, hip as H
    from pydreamer_amd.models import Dreamer
    oconf = O.make_conf(deter_dim=600, hidden_dim=1000, stoch_dim=32, stoch_discrete=32, cnn_depth=8, action_dim=18,
                        batch_size=4, batch_length=4, imag_horizon=5)
    params = O.make_params(oconf, seed=2)
    conf = config.load_config('defaults', 'atari', **{**{k: getattr(oconf, k) for k in vars(oconf)}, 'amp': True})
    model = Dreamer(conf)
    model.load_state_dict(params, strict=True)
    model = model.to(DEV)
    M, Hh = 300, 5
    g = torch.Generator().manual_seed(5)
    h = torch.tanh(torch.randn(M, 600, generator=g)).to(DEV)
    z = F.one_hot(torch.randint(0, 32, (M, 32), generator=g), 32).float().reshape(M, -1).to(DEV)
    u_act, u_prior = torch.rand(Hh, M, generator=g).to(DEV), torch.rand(Hh, M, 32, generator=g).to(DEV)
    out = []
    try:
        for on in (1, 0):
            H.lib().dm_bf16_twins_enable(on)
            fh, ah, rh, th = model.dream((h, z), Hh, u_act=u_act, u_prior=u_prior)
            out.append((fh.clone(), ah.clone()))
    finally:
        H.lib().dm_bf16_twins_enable(1)
    (f1, a1), (f0, a0) = out
    assert torch.isfinite(f1).all()
    same = (a1 == a0).all(dim=-1).reshape(Hh, M)
    assert float(same.float().mean()) > 0.995        # a sample within fp32 rounding of a CDF edge may flip (and changes what follows)
    rows = same.all(dim=0)                             # trajectories with identical actions throughout
    zsame = (f1[:, :, 600:] == f0[:, :, 600:]).all(dim=-1).all(dim=0) & rows
    assert float(zsame.float().mean()) > 0.9
    _close(f1[:, zsame], f0[:, zsame], 0, 2e-5, 'dream features, twins on vs off')


@pytest.mark.parametrize('B,D_', [(6, 600), (7, 600), (13, 600), (25, 600), (50, 600), (64, 600), (32, 1024)])
def test_rssm_lds_chain_matches_launch_schedule(hip, B, D_):
    """The posterior T loop as ONE persistent kernel whose workgroups keep the cell's weight slices in LDS (csrc/rssm_lds.hip:
    one workgroup per CU on all XCDs, activation rows exchanged through poison-filled per-step buffers) against the
    five-launch fused schedule it replaces, at the Atari-literal cell width, T = 12, for the row counts of a 1 / 2 / 4 / 8-way
    batch shard (50, 25, 13, 7 / 6; one lane group layout each: 64, 32, 16, 8 rows per k-group) and a full 64.  Same
    arithmetic up to fp32 summation order (K is split over waves and k-groups differently), same sampler rule: sampled
    indices equal (a uniform within an ulp of a CDF edge excepted: >= 99.9 %), logits / states / saved activations within
    2e-5 + 1e-5 relative of the launch schedule on the rows whose history of indices is identical; the kernel never gave up
    in a spin loop.  (32, 1024) is pydreamer's own shipped Atari cell (defaults+atari: B = 32, deter_dim 1024): its slices fill a
    CU's LDS only with z_mlp^T left in L2 (`wz_global`).  (Parity with the reference itself: test_rssm_sequence_fwd_bwd_vs_oracle
    and both full-size golden replays run this kernel too.)"""
    import ctypes
    from pydreamer_amd import hip as H
    T, Hd, S, C, A, depth = 12, 1000, 32, 32, 18, 8
    oconf = O.make_conf(deter_dim=D_, hidden_dim=Hd, stoch_dim=S, stoch_discrete=C, cnn_depth=depth, action_dim=A,
                        batch_size=B, batch_length=T)
    model = _build(oconf, O.make_params(oconf, seed=4))
    cell = model.wm.core.cell
    E, Z, F_ = 32 * depth, S * C, D_ + S * C
    g = torch.Generator().manual_seed(12)
    embed = torch.randn(T * B, E, generator=g).to(DEV)
    action = F.one_hot(torch.randint(0, A, (T * B,), generator=g), A).float().to(DEV)
    reset = (torch.rand(T * B, generator=g) < 0.1).to(torch.uint8).to(DEV)
    h0, z0 = torch.tanh(torch.randn(B, D_, generator=g)).to(DEV), torch.zeros(B, Z).to(DEV)
    u = torch.rand(T * B, S, generator=g).to(DEV)
    shp = model.wm.shape(T, B, 1)
    ws = model.wm.workspace(shp, torch.device(DEV, 0))
    P = H.rssm_struct(cell.ordered())
    outs = []
    assert H.lib().dm_rssm_lds_status() == 0
    try:
        for on in (2, 0):      # (level 2: the default level leaves B > 32 to the launch chain, which is faster there)
            H.lib().dm_rssm_lds_enable(on)
            acts = torch.zeros(int(H.lib().dm_rssm_acts_floats(ctypes.byref(shp))), device=DEV)
            feat, post, prior = torch.zeros(T * B, F_, device=DEV), torch.zeros(T * B, Z, device=DEV), torch.zeros(T * B, Z, device=DEV)
            idx = torch.zeros(T * B, S, dtype=torch.int32, device=DEV)
            for rep in range(2):      # twice: the second call runs with L1 / L2 warm on the same exchange addresses
                H.call('dm_rssm_sequence_fwd', ctypes.byref(shp), H.fptr(embed), H.fptr(action), H.ptr(reset), H.fptr(h0), H.fptr(z0),
                       H.fptr(u), None, ctypes.byref(P), H.fptr(acts), H.fptr(feat), H.fptr(post), H.fptr(prior), H.ptr(idx),
                       H.ptr(ws), ws.numel(), H.stream())
                torch.cuda.synchronize()
            outs.append((feat, post, prior, idx, acts))
    finally:
        H.lib().dm_rssm_lds_enable(1)
    assert H.lib().dm_rssm_lds_status() == 0, 'the persistent kernel gave up in a spin loop'
    same = (outs[0][3] == outs[1][3]).view(T, B, S)
    print(f'B={B}: indices equal {float(same.float().mean()):.6f}')
    assert float(same.float().mean()) >= 0.999
    # rows whose indices agree at every step so far carry the same state; a flipped draw legitimately changes what follows
    ok_rows = same.all(dim=2).cummin(dim=0).values.reshape(T * B)
    assert float(ok_rows.float().mean()) >= 0.97
    for a, b, what in zip(outs[0][:3], outs[1][:3], ('feat', 'post', 'prior')):
        assert torch.isfinite(a).all(), what
        err = (a[ok_rows] - b[ok_rows]).abs()
        assert float((err - 1e-5 * b[ok_rows].abs()).max()) <= 2e-5, (what, float(err.max()))
    # saved activations (what the backward pass reads): the whole arena, rows with an identical history
    RA, N = outs[0][4], T * B
    RB = outs[1][4]
    assert torch.isfinite(RA).all()
    off = 0
    for name, width in (('ea', Hd), ('ee', Hd), ('hin', D_), ('zin', Z), ('x1', Hd), ('st1', 2), ('za', Hd), ('gi', 3 * D_), ('gh', 3 * D_),
                        ('x2', Hd), ('st2', 2), ('pin', Hd)):
        a = RA[off:off + N * width].view(N, width)[ok_rows]
        b = RB[off:off + N * width].view(N, width)[ok_rows]
        err = (a - b).abs()
        assert float((err - 2e-5 * b.abs()).max()) <= 5e-5, (name, float(err.max()))
        off += (N * width + 63) // 64 * 64      # the arena is carved in 64-float granules (csrc/common.h DmArena)


def test_rssm_lds_kernel_with_a_busy_chip(hip):
    """The persistent posterior kernel needs one workgroup resident on every CU at the same time.  The library checks with the
    occupancy API that the grid CAN be co-resident (csrc/rssm_lds.hip rl_raise_lds / rl_device_ok) and its spin loops are
    bounded; this test runs it while a second stream keeps every CU busy with LDS-heavy work - a queue of 4096^3
    products on 128 x 128 tiles, 64 KiB of LDS per workgroup, two per CU, ~1 ms each - so that its workgroups become
    resident one by one as the tiles of the other stream retire, and the early ones wait for the late ones.  Asserted: the
    kernel never gives up (dm_rssm_lds_status() == 0) and every output equals the quiet run's BIT FOR BIT (the exchange
    protocol makes the arithmetic independent of arrival order)."""
    import ctypes
    from pydreamer_amd import hip as H
    T, B, D_, Hd, S, C, A, depth = 12, 13, 600, 1000, 32, 32, 18, 8
    oconf = O.make_conf(deter_dim=D_, hidden_dim=Hd, stoch_dim=S, stoch_discrete=C, cnn_depth=depth, action_dim=A,
                        batch_size=B, batch_length=T)
    model = _build(oconf, O.make_params(oconf, seed=4))
    cell = model.wm.core.cell
    E, Z, F_ = 32 * depth, S * C, D_ + S * C
    g = torch.Generator().manual_seed(13)
    embed = torch.randn(T * B, E, generator=g).to(DEV)
    action = F.one_hot(torch.randint(0, A, (T * B,), generator=g), A).float().to(DEV)
    reset = (torch.rand(T * B, generator=g) < 0.1).to(torch.uint8).to(DEV)
    h0, z0 = torch.tanh(torch.randn(B, D_, generator=g)).to(DEV), torch.zeros(B, Z).to(DEV)
    u = torch.rand(T * B, S, generator=g).to(DEV)
    shp = model.wm.shape(T, B, 1)
    ws = model.wm.workspace(shp, torch.device(DEV, 0))
    P = H.rssm_struct(cell.ordered())
    n = 4096
    ga, gb, gc = torch.randn(n, n, device=DEV), torch.randn(n, n, device=DEV), torch.empty(n, n, device=DEV)
    gws = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    clk = (ctypes.c_ulonglong * 16)()
    H.lib().dm_rssm_lds_prof(clk, 1)
    assert H.lib().dm_rssm_lds_status() == 0 and H.lib().dm_rssm_lds_enable(-1) >= 1
    outs = []
    for busy in (False, True):
        acts = torch.zeros(int(H.lib().dm_rssm_acts_floats(ctypes.byref(shp))), device=DEV)
        feat, post, prior = torch.zeros(T * B, F_, device=DEV), torch.zeros(T * B, Z, device=DEV), torch.zeros(T * B, Z, device=DEV)
        idx = torch.zeros(T * B, S, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        if busy:
            with torch.cuda.stream(side):
                for _ in range(40):      # ~45 ms of back-to-back tiles on the other stream; the sequence below is ~1 ms of work
                    H.call('dm_gemm_f32', 0, 0, n, n, n, H.fptr(ga), n, H.fptr(gb), n, H.fptr(gc), n, None, None, 0, 0,
                           H.ptr(gws), gws.numel(), ctypes.c_void_p(side.cuda_stream))
        H.call('dm_rssm_sequence_fwd', ctypes.byref(shp), H.fptr(embed), H.fptr(action), H.ptr(reset), H.fptr(h0), H.fptr(z0),
               H.fptr(u), None, ctypes.byref(P), H.fptr(acts), H.fptr(feat), H.fptr(post), H.fptr(prior), H.ptr(idx),
               H.ptr(ws), ws.numel(), H.stream())
        torch.cuda.synchronize()
        outs.append((feat, post, prior, idx))
    H.lib().dm_rssm_lds_prof(clk, 0)
    assert sum(clk) > 0, 'the persistent posterior kernel did not run (13 rows at deter 600 is inside its default range)'
    assert H.lib().dm_rssm_lds_status() == 0, 'the persistent kernel gave up in a spin loop while the other stream held CUs'
    for a, b, what in zip(outs[0], outs[1], ('feat', 'post', 'prior', 'idx')):
        assert torch.equal(a, b), what


MID = dict(deter_dim=256, hidden_dim=256, stoch_dim=8, stoch_discrete=32)      # the smallest width at which every <= 64-row product of a step reaches the fused schedules' 64K floor


@contextlib.contextmanager
def _record_schedules():
    """dm_rssm_last_schedule() of every dm_rssm_sequence_fwd / _bwd / dm_dream_rollout call made inside the block, read on the
    thread that made the call (the word is thread-local, and the model's backward runs on an autograd or launcher thread)."""
    from pydreamer_amd import hip as H
    which = {'dm_rssm_sequence_fwd': 0, 'dm_rssm_sequence_bwd': 1, 'dm_dream_rollout': 2}
    seen, real = {'fwd': [], 'bwd': [], 'rollout': []}, H.call

    def call(name, *args):
        rc = real(name, *args)
        if name in which:
            seen[('fwd', 'bwd', 'rollout')[which[name]]].append(H.last_schedule(which[name]))
        return rc
    H.call = call
    try:
        yield seen
    finally:
        H.call = real


def _assert_schedule(seen, **want):
    """want: fwd / bwd / rollout -> dict of bits the FIRST such call of the block must report (keys left out are not asserted)."""
    for entry, bits in want.items():
        assert seen[entry], f'no {entry} call was recorded'
        got = seen[entry][0]
        for k, v in bits.items():
            assert got[k] == v, f'{entry}: schedule bit {k} is {got[k]}, expected {v} (reported {got})'


def _mid_schedule(B, T, Hh, rows, sample=True, fold_sm=True, psync=False):
    """The schedule a trainer iteration must report at a width like MID, read from the predicates of csrc/rssm.hip: <= 64 posterior
    rows take the fused forward and the folded backward; the rollout's actor runs on the whole-MLP kernel from 256 rows up."""
    fused = B <= 64
    return dict(fwd=dict(fuse_ln=fused, fuse_sample=fused and sample, frag=fused and sample, wzt=T > 1, psync=psync),
                bwd=dict(fuse_b=fused, fold=fused, fold_sm=fused and fold_sm, frag=fused, nchunk=1 if (B < 16 or T < 8) else (2 if T < 16 else 4)),
                rollout=dict(wzt=Hh > 1, wat=Hh > 1, actor_wpack=rows >= 256, actor_add0=rows >= 256 and Hh > 1, fuse_act=rows >= 256,
                             tw_on=False))


PLAIN_SCHEDULE = dict(fwd=dict(fuse_ln=False, fuse_sample=False, frag=False, psync=False), bwd=dict(fuse_b=False, fold=False, fold_sm=False, frag=False))


def _run_pair(oconf, steps, forced=False, seed=0, mutate=None, expect=None):
    """One or more full trainer iterations (train.py:165-198) on the oracle (CPU) and the HIP model (GPU).  expect: the launch
    schedule (_assert_schedule's arguments) the first iteration must report - asserted before anything is compared."""
    params = O.make_params(oconf, seed=seed)
    ora = O.OracleDreamer(oconf, params)
    ora.init_optimizers()
    model = _build(oconf, params)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    st_o = ora.init_state(oconf.batch_size * oconf.iwae_samples)       # IWAE: B*I state rows, row b*I + i (rssm.py:35-41)
    st_h = model.init_state(oconf.batch_size * oconf.iwae_samples)
    out = []
    for s in range(steps):
        raw = O.synthetic_batch(oconf, seed=1234 + s, first=(s == 0))
        if mutate is not None:
            mutate(raw, s)
        noise = O.make_noise(oconf, seed=777 + s)
        obs = O.preprocess(raw, oconf)
        lo, st_o2, mo, to, xo = ora.training_step(obs, st_o, noise)
        gmo, go = ora.backward_clip_step(lo)
        fidx = xo['post_idx'].reshape(oconf.batch_length, oconf.batch_size * oconf.iwae_samples, -1).to(DEV) if forced else None
        with _record_schedules() as seen:
            lh, st_h2, mh, th, _ = model.training_step(_to_dev(obs), st_h, noise=_to_dev(noise), forced_idx=fidx)
            for opt in opts:
                opt.zero_grad()
            for loss in lh:
                loss.backward()
            gmh = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        if expect is not None and s == 0:
            print('SCHEDULE', {k: v[0] for k, v in seen.items() if v})
            _assert_schedule(seen, **expect)
        # like the oracle's, gradients are compared AFTER clip_grad_norm_ scaled them in place (norm > 200 for some seeds)
        gh = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None and v.requires_grad}
        for opt in opts:
            opt.step()
        # last_extras' large entries are the step's own buffers, not copies: snapshot them
        xh = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in model.last_extras.items()}
        out.append(dict(lo=lo, lh=lh, mo={**mo, **gmo}, mh={**mh, **gmh}, to=to, th=th, xo=xo, xh=xh,
                        go=go, gh=gh, st_o=st_o2, st_h=st_h2,
                        po={k: v.detach().clone() for k, v in ora.p.items()},
                        ph={k: v.detach().clone() for k, v in model.state_dict().items()}))
        st_o, st_h = st_o2, st_h2
    return out


def _check_pair(r, oconf, free_running=True):
    T, B, S = oconf.batch_length, oconf.batch_size * oconf.iwae_samples, oconf.stoch_dim      # posterior rows: B*I under IWAE
    if free_running:
        pi_h = r['xh']['post_idx'].cpu().long().reshape(T, B, S)
        pi_o = r['xo']['post_idx'].reshape(T, B, S)
        assert torch.equal(pi_h, pi_o), f'{int((pi_h != pi_o).sum())} posterior index mismatches'
        if oconf.actor_dist == 'onehot':
            assert torch.equal(r['xh']['act_idx'].cpu().long(), r['xo']['act_idx']), 'dream action index mismatch'
        else:
            _close(r['xh']['actions'], r['xo']['actions'], 1e-4, 1e-5, 'dream continuous actions')
        if oconf.stoch_discrete:
            lat_h = r['xh']['dream_features'][1:, :, oconf.deter_dim:].reshape(oconf.imag_horizon, -1, S, oconf.stoch_discrete).argmax(-1).cpu()
            assert torch.equal(lat_h, r['xo']['lat_idx']), 'dream latent index mismatch'
    names = ('loss_model', 'loss_probe', 'loss_actor', 'loss_critic')
    for n, a, b in zip(names, r['lh'], r['lo']):
        assert _rel(a, b) < 2e-5 or abs(float(a) - float(b)) < 2e-6, (n, float(a), float(b))
    assert abs(float(r['lh'][0]) - float(r['lo'][0])) < 1e-3, 'north-star bar: loss_model within 1e-3 of the reference path'
    for k, v in r['mo'].items():
        assert _rel(r['mh'][k], v) < 1e-4 or abs(float(r['mh'][k]) - float(v)) < 5e-6, (k, float(r['mh'][k]), float(v))
    for k, v in r['to'].items():
        _close(r['th'][k], v, 1e-4, 1e-4 * max(1.0, float(v.abs().max())), f'tensor {k}')
    _close(r['st_h'][0], r['st_o'][0], 0, 1e-5, 'out_state h')
    if oconf.stoch_discrete:
        assert torch.equal(r['st_h'][1].cpu(), r['st_o'][1]), 'out_state z'
    else:       # Gaussian latents: z is a float sample
        _close(r['st_h'][1], r['st_o'][1], 0, 2e-5, 'out_state z')
    worst = ('', 0.0)
    for k, g in r['go'].items():
        e = _rel_l2(r['gh'][k], g)
        if e > worst[1]:
            worst = (k, e)
    assert worst[1] < 2e-3, f'gradient rel-L2 error {worst[1]:.2e} at {worst[0]}'
    for k, v in r['po'].items():
        _close(r['ph'][k], v, 0, 1e-5, f'post-AdamW {k}')


def test_training_step_tiny_two_steps_vs_oracle(hip):
    """Free-running (sampling on the GPU from the shared uniforms), 2 steps with TBTT state carry and the
    critic_target refresh at call 0."""
    oconf = O.tiny_conf()
    for r in _run_pair(oconf, 2):
        _check_pair(r, oconf)


@pytest.mark.parametrize('B,T,Hh', [(1, 2, 1), (1, 5, 4), (16, 2, 2), (17, 3, 2), (32, 2, 2), (33, 2, 2), (51, 5, 2), (64, 4, 2), (65, 4, 3)])
def test_training_step_at_dispatch_boundaries_vs_oracle(hip, B, T, Hh):
    """Batch / sequence sizes on both sides of every row threshold the host and the library dispatch on: one batch column and the
    shortest sequence with a transition (B = 1, T = 2, H = 1); 16 / 17 and 32 / 33 rows (strip heights of the <= 64-row products,
    the persistent posterior kernel's <= 32-row limit); 64 / 65 rows (strip kernels vs tile kernels in the T loops); T x B = 255 /
    256 / 260 imagination rows (launch chain vs whole-MLP kernel).  Two consecutive trainer iterations each, every loss, metric,
    sampled index, per-parameter gradient and post-AdamW parameter against the oracle."""
    oconf = O.tiny_conf(batch_size=B, batch_length=T, imag_horizon=Hh)
    for r in _run_pair(oconf, 2, seed=B + T):
        _check_pair(r, oconf)


@pytest.mark.parametrize('B,T,Hh,seed', [(1, 2, 1, 3), (16, 2, 2, 18), (17, 3, 2, 20), (32, 2, 2, 36), (33, 2, 2, 35), (64, 4, 2, 68), (65, 4, 3, 80)])
def test_training_step_at_dispatch_boundaries_mid_width_vs_oracle(hip, B, T, Hh, seed):
    """The sibling of test_training_step_at_dispatch_boundaries_vs_oracle at deter 256 / hidden 256 / stoch 8x32, where the row
    thresholds are those of the FUSED schedules (at the tiny width 3 D Hd = 12 288 is under the 64K floor of every fused path, so the
    tiny test walks the plain 8-launch schedule only): LayerNorm+ELU in prologues / in the z_embed gather, the sampler epilogue,
    fragment copies, the folded LayerNorm backward with fold_sm up to 64 rows, everything plain at 65; the rollout's and the heads'
    <= 64-row products over the 512-wide feature on the skinny kernel (400 x 512 >= 64K), the whole-MLP actor with its gathered
    first layer from 256 imagination rows.  The schedule of the first iteration is asserted (fwd, bwd, rollout), then two
    iterations meet all of _check_pair's bars.
    Seeds chosen on the CPU (oracle alone, candidates B + T ...): the first whose posterior, prior and action draws of both
    iterations all stay >= 2e-6 from an fp32-oracle CDF edge.  Minimum distances at the chosen seeds: (1,2,1) 3.3e-4, (16,2,2)
    3.4e-6, (17,3,2) 1.4e-5, (32,2,2) 3.9e-6 (seeds 34 / 35: 4.8e-7 / 3.6e-7), (33,2,2) 5.0e-6, (64,4,2) 2.2e-6, (65,4,3) 3.8e-6
    (seeds 69..79: 2.3e-7 .. 1.3e-6)."""
    oconf = O.tiny_conf(batch_size=B, batch_length=T, imag_horizon=Hh, **MID)
    for r in _run_pair(oconf, 2, seed=seed, expect=_mid_schedule(B, T, Hh, T * B)):
        _check_pair(r, oconf)


NON_DEFAULT_BOUNDARY_CASES = [
    # Gaussian latents: posterior rows 17 / 32 / 33 / 65, imagination rows T x B = 255 / 256 / 66 / 260
    dict(stoch_discrete=0, batch_size=17, batch_length=15), dict(stoch_discrete=0, batch_size=32, batch_length=8),
    dict(stoch_discrete=0, batch_size=33, batch_length=2), dict(stoch_discrete=0, batch_size=65, batch_length=4),
    # continuous actors, action_dim 1 and 12, imagination rows 255 / 256 / 260
    dict(actor_dist='tanh_normal', action_dim=1, batch_size=17, batch_length=15),
    dict(actor_dist='tanh_normal', action_dim=12, batch_size=65, batch_length=4),
    dict(actor_dist='normal_tanh', action_dim=12, batch_size=17, batch_length=15),
    dict(actor_dist='normal_tanh', action_dim=1, batch_size=32, batch_length=8),
]


def _case_id(kw):
    fam = 'actor' if 'actor_dist' in kw else 'gauss'
    parts = [fam] + [f'{k}={v}' for k, v in kw.items() if k not in ('batch_size', 'batch_length')]
    return '-'.join(parts) + f'-B{kw["batch_size"]}-T{kw["batch_length"]}'


@pytest.mark.parametrize('kw', NON_DEFAULT_BOUNDARY_CASES, ids=[_case_id(k) for k in NON_DEFAULT_BOUNDARY_CASES])
def test_non_default_configs_at_dispatch_boundaries_vs_oracle(hip, kw):
    """The sibling of test_training_step_at_dispatch_boundaries_vs_oracle for the configurations off the default path:
    Gaussian latents (stoch_discrete = 0) and the tanh_normal / normal_tanh actors with one and twelve action dimensions, each
    at posterior-row counts around 16 / 32 / 64 and imagination row counts T x B of 255 / 256 / 260.  Two consecutive trainer
    iterations, all of _check_pair's bars."""
    kw = dict(kw)
    if 'actor_dist' in kw:
        kw.setdefault('entropy', 1.0e-4)
    oconf = O.tiny_conf(imag_horizon=2, **kw)
    for r in _run_pair(oconf, 2, seed=kw['batch_size'] + kw['batch_length']):
        _check_pair(r, oconf)


def _all_reset(raw, s):
    raw['reset'][:] = True


def _no_reset(raw, s):
    raw['reset'][:] = False


def _all_terminal(raw, s):
    raw['terminal'][:] = 1.0
    raw['reward'][:] = 1.0


def _extreme_frames(raw, s):
    raw['image_u8'][:] = 255 if s == 0 else 0
    raw['reward'][:] = -1.0
    raw['action_idx'][:] = raw['action_idx'].max()


@pytest.mark.parametrize('mutate,mid', [pytest.param(_all_reset, False, id='all_reset'), pytest.param(_no_reset, False, id='no_reset'),
                                        pytest.param(_all_terminal, False, id='all_terminal'), pytest.param(_extreme_frames, False, id='extreme_frames'),
                                        pytest.param(_all_reset, True, id='all_reset-mid'), pytest.param(_no_reset, True, id='no_reset-mid')])
def test_training_step_on_degenerate_batches_vs_oracle(hip, mutate, mid):
    """Replay batches at the corners of what preprocessing can hand over (preprocessing.py:135-150): every row reset at every step
    (the recurrent state is zeroed before each cell, rssm.py:117-119), no reset at all (two iterations: the second starts from the
    carried state), every step terminal with reward 1, saturated frames (all 255, then all 0) with one repeated action and reward
    -1.  Two trainer iterations each against the oracle, all of _check_pair's bars.
    `-mid`: all / no reset again at deter 256 / hidden 256 / stoch 8x32, schedule asserted: there the masks are `row_zero` options
    inside the fused schedules' products, not the mask kernels of the plain path (seed 11: every draw >= 7.0e-6 from an
    fp32-oracle CDF edge in both cases)."""
    oconf = O.tiny_conf(batch_size=4, batch_length=6, imag_horizon=3, **(MID if mid else {}))
    for r in _run_pair(oconf, 2, seed=11, mutate=mutate, expect=_mid_schedule(4, 6, 3, 24) if mid else PLAIN_SCHEDULE):
        _check_pair(r, oconf)


def test_training_step_teacher_forced_vs_oracle(hip):
    """Posterior indices forced to the oracle's: isolates float parity from sampler decisions."""
    oconf = O.tiny_conf(batch_size=4, batch_length=6, kl_balance=0.5)     # also covers the plain-KL branch (dreamer.py:334-335)
    for r in _run_pair(oconf, 1, forced=True, seed=1):
        _check_pair(r, oconf, free_running=False)


def test_training_step_continuous_actor_vs_oracle(hip):
    """DMC-style Gaussian actors (BASELINE configs[4] family): tanh_normal and normal_tanh with actor_grad=reinforce."""
    for dist in ('tanh_normal', 'normal_tanh'):
        oconf = O.tiny_conf(actor_dist=dist, action_dim=4, entropy=1.0e-4, gamma=0.995)
        for r in _run_pair(oconf, 1):
            _check_pair(r, oconf)


@pytest.mark.parametrize('stoch,classes,mid', [pytest.param(40, 32, False, id='40-32'), pytest.param(64, 32, False, id='64-32'),
                                               pytest.param(33, 8, False, id='33-8'), pytest.param(40, 32, True, id='40-32-mid'),
                                               pytest.param(16, 16, True, id='16-16-mid')])
def test_training_step_wide_stoch_vs_oracle(hip, stoch, classes, mid):
    """stoch_dim > 32 (the reference's larger configurations, e.g. 96 x 32 with deter 2048) and class counts other than 32: every
    loss, metric and per-parameter gradient of two consecutive steps against the oracle, at two dm_rssm_lds_enable levels, with
    the schedule of each run asserted.  What each parameter runs:
      40-32, 64-32, 33-8 (hidden 64): the plain 8-launch schedule in both directions - no fused path is selected under the 64K
        floor - with the generic sampler and z_mlp kernels over more than 32 latents per row.  The persistent kernel is refused at
        level 1 and at level 0 alike: its slices need under 80 KiB of LDS (only level 2 takes such a model), and for 40 / 64 x 32
        its plan has S*C/4 > 256 workgroups at any width.
      40-32-mid (deter 256, hidden 256): S > 32 at a fused width - the sampler epilogue over 40 groups, the gate product's
        prologue form at every step (the row-per-workgroup gather holds <= 32 groups: no `ln_z`), fuse_b + fold + fold_sm at
        N = 1280; persistent kernel refused at levels 1 and 0 (320 workgroups).
      16-16-mid: fuse_ln without the sampler epilogue and without fragment copies, fold without fold_sm; levels 2 and 0 - at
        level 2 the persistent kernel takes steps 1.. (C = 16).
    Seed 0: every posterior, prior and action draw of both iterations stays >= 2.7e-6 (40-32-mid) / 3.8e-5 (16-16-mid) from an
    fp32-oracle CDF edge."""
    from pydreamer_amd import hip as H
    oconf = O.tiny_conf(stoch_dim=stoch, stoch_discrete=classes, **(dict(deter_dim=256, hidden_dim=256) if mid else {}))
    B, T, Hh = oconf.batch_size, oconf.batch_length, oconf.imag_horizon
    levels = (2, 0) if (mid and classes == 16) else (1, 0)
    keep = H.lib().dm_rssm_lds_enable(-1)
    try:
        for lds in levels:
            H.lib().dm_rssm_lds_enable(lds)
            expect = PLAIN_SCHEDULE
            if mid:
                expect = _mid_schedule(B, T, Hh, T * B, sample=classes == 32, fold_sm=classes == 32, psync=lds == 2)
            for r in _run_pair(oconf, 2, expect=expect):
                _check_pair(r, oconf)
    finally:
        H.lib().dm_rssm_lds_enable(keep)


@pytest.mark.parametrize('layers,deter', [(2, 64), (4, 96)])
def test_training_step_gru_cell_stack_vs_oracle(hip, layers, deter):
    """GRUCellStack with several layers (rnn.py:40-67) against the oracle: every loss, metric and per-parameter gradient
    of two consecutive steps (resets included)."""
    oconf = O.tiny_conf(gru_layers=layers, deter_dim=deter)
    for r in _run_pair(oconf, 2):
        _check_pair(r, oconf)


@pytest.mark.parametrize('gru_type,layers,deter', [('gru_layernorm', 2, 64), ('gru_layernorm_dv2', 2, 64), ('gru_layernorm', 3, 96),
                                                   ('gru_layernorm_dv2', 4, 96)])
def test_training_step_layernorm_cell_stack_vs_oracle(hip, gru_type, layers, deter):
    """GRUCellStack of the LayerNorm cells (rnn.py:51-57 with rnn.py:95-138): per-layer LayerNorm parameters, no gate biases;
    every loss, metric and per-parameter gradient of two consecutive steps."""
    oconf = O.tiny_conf(gru_type=gru_type, gru_layers=layers, deter_dim=deter)
    for r in _run_pair(oconf, 2):
        _check_pair(r, oconf)


@pytest.mark.parametrize('kw', [dict(), dict(actor_dist='tanh_normal', action_dim=4, entropy=1.0e-4), dict(gru_type='gru_layernorm')])
def test_training_step_no_layernorm_vs_oracle(hip, kw):
    """layer_norm=False (common.py:68-74 NoNorm in every MLP head and in the RSSM cell's three norms; the GRU cell's own
    LayerNorms are a separate switch): every loss, metric and per-parameter gradient of two consecutive steps."""
    oconf = O.tiny_conf(layer_norm=False, **kw)
    for r in _run_pair(oconf, 2):
        _check_pair(r, oconf)


@pytest.mark.parametrize('kw', [dict(), dict(layer_norm=False, gru_type='gru_layernorm_dv2'),
                                dict(actor_dist='tanh_normal', action_dim=4, entropy=1.0e-4, kl_balance=0.5, gru_layers=2)])
def test_training_step_gaussian_latents_vs_oracle(hip, kw):
    """stoch_discrete = 0 (rssm.py:103-117,195-203; functions.py:46-56): Gaussian latents - reparameterised posterior and
    prior samples, the Normal KL (balanced and plain), entropies, BPTT through mean and std - two consecutive steps, every
    loss, metric and per-parameter gradient."""
    oconf = O.tiny_conf(stoch_discrete=0, **kw)
    for r in _run_pair(oconf, 2):
        _check_pair(r, oconf)


def test_training_step_matches_reference_goldens(hip):
    """Directly against the fixtures written by the real reference (tests/golden/tiny.npz, debug_literal.npz, tiny_dmc.npz,
    the LayerNorm GRU cells of rnn.py:95-138: tiny_gru_layernorm.npz, tiny_gru_layernorm_dv2.npz, and the auxiliary critic
    of dreamer.py:267-279,347-358: tiny_aux_critic.npz, and the 3-layer GRUCellStack of rnn.py:40-67: tiny_gru_layers3.npz -
    SURVEY 8(f) N4; layer_norm=False, common.py:68-74 NoNorm: tiny_no_layernorm.npz; Gaussian latents, stoch_discrete=0,
    rssm.py:195-203: tiny_gaussian_latents.npz; a 2-layer stack of NormGRUCells: tiny_gru_layernorm_layers2.npz; the
    normal_tanh actor of functions.py:59-66: tiny_normal_tanh.npz; the plain-KL branch kl_balance = 0.5 of dreamer.py:241,334-335:
    tiny_kl_plain.npz; every scalar hyper-parameter off its default with binding gradient clips, 3 steps: tiny_scalars.npz;
    probe_gradients=True - three optimizers, summed first loss, dreamer.py:60-87,183-186: tiny_probe_gradients.npz)."""
    for name, steps in (('tiny', 2), ('debug_literal', 1), ('tiny_dmc', 1), ('tiny_gru_layernorm', 2),
                        ('tiny_gru_layernorm_dv2', 2), ('tiny_aux_critic', 2), ('tiny_gru_layers3', 2), ('tiny_no_layernorm', 2),
                        ('tiny_gaussian_latents', 2), ('tiny_gru_layernorm_layers2', 1), ('tiny_normal_tanh', 2), ('tiny_kl_plain', 2),
                        ('tiny_scalars', 3), ('tiny_probe_gradients', 2)):
        _check_reference_golden(name, steps)


def test_combined_variants_match_reference_golden(hip):
    """tests/golden/tiny_combo.npz: the structural variants TOGETHER (Gaussian latents, a 2-layer stack of late-reset LayerNorm GRU
    cells, NoNorm MLPs, the auxiliary critic, a tanh_normal actor on continuous actions) - their interaction, not each alone."""
    _check_reference_golden('tiny_combo', 2)


def _check_reference_golden(name, steps):
    """One fixture written by the real reference (oracle/gen_golden.py) replayed through the HIP path: sampled indices bit-exact,
    losses / metrics / gradient norms (after the clip, like the fixture's) / post-AdamW parameter checksums at the bars below."""
    g = np.load(os.path.join(GOLD, f'{name}.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    params = O.make_params(oconf, seed=0)
    model = _build(oconf, params)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    state = model.init_state(oconf.batch_size)
    T, B, S = oconf.batch_length, oconf.batch_size, oconf.stoch_dim
    for s in range(steps):
        pre = f's{s}_'
        raw = {k: g[pre + 'in_' + k] for k in ('image_u8', 'action_idx', 'reward', 'terminal', 'reset')}
        obs = _to_dev(O.preprocess(raw, oconf))
        noise = {k: torch.from_numpy(g[pre + 'in_' + k]).to(DEV) for k in ('u_post', 'u_act', 'u_prior', 'eps_act')
                 if pre + 'in_' + k in g.files}
        losses, state, metrics, tensors, _ = model.training_step(obs, state, noise=noise)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        for opt in opts:
            opt.step()
        assert np.array_equal(model.last_extras['post_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_post']), name
        if oconf.actor_dist == 'onehot':
            assert np.array_equal(model.last_extras['act_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_act']), name
        for i, l in enumerate(losses):
            ref = g[pre + 'losses'][i]
            assert _rel(l, ref) < 2e-5 or abs(float(l) - ref) < 2e-6, (name, s, i, float(l), ref)
        assert abs(float(losses[0]) - g[pre + 'losses'][0]) < 1e-3
        for k, v in {**metrics, **gm}.items():
            ref = float(g[pre + 'metric_' + k])
            assert _rel(v, ref) < 1e-4 or abs(float(v) - ref) < 5e-6, (name, s, k, float(v), ref)
        names = [str(n) for n in g[pre + 'grad_names']]
        named = dict(model.named_parameters())
        for n, ref in zip(names, g[pre + 'grad_norms']):
            got = float(named[n].grad.double().norm())     # (after the clip, like the fixture's: it binds in tiny_scalars only)
            assert abs(got - ref) <= 2e-3 * ref + 1e-7, (name, s, n, got, ref)
        sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
        np.testing.assert_allclose(sums, g[pre + 'param_abs_sums'], rtol=2e-6)


@pytest.mark.parametrize('name,steps', [('tiny', 2), ('tiny_aux_critic', 2), ('tiny_scalars', 3), ('tiny_kl_plain', 2)])
def test_reference_goldens_through_the_persistent_chain_kernels(hip, name, steps):
    """The fixtures written by the real reference replayed with the persistent posterior kernel forced on (csrc/rssm_lds.hip;
    switch level 2 admits models whose weight slices need less than half a CU's LDS, which
    the default leaves to the launch chain): sampled indices bit-exact, losses / metrics / gradient norms / post-AdamW parameter
    checksums at the same bars as the launch schedule - incl. two consecutive steps with the carried state, binding gradient
    clips and off-default loss weights (tiny_scalars), the un-balanced KL, the auxiliary critic.  (debug_literal and the two full-size
    fixtures have deter_dim 1024 / 600: the first does not fit a CU's LDS and stays on the launch chain, the second runs the
    posterior kernel by default in test_training_step_matches_reference_at_atari_literal.)"""
    from pydreamer_amd import hip as H
    lib = H.lib()
    was = lib.dm_rssm_lds_enable(-1)
    lib.dm_rssm_lds_enable(2)
    try:
        out = (ctypes_ull16 := (__import__('ctypes').c_ulonglong * 16)())
        lib.dm_rssm_lds_prof(out, 1)                  # (allocates and zeroes the phase clocks: non-zero afterwards = the kernel ran)
        _check_reference_golden(name, steps)
        torch.cuda.synchronize()
        lib.dm_rssm_lds_prof(ctypes_ull16, 0)
        assert sum(ctypes_ull16) > 0, 'the persistent posterior kernel did not run'
        assert lib.dm_rssm_lds_status() == 0
    finally:
        lib.dm_rssm_lds_enable(was)


def test_gaussian_latents_iwae_matches_reference_golden(hip):
    """stoch_discrete = 0 WITH iwae_samples = 2 (dreamer.py:340-343 with rssm.py:202-203: the sampled KL is a difference of
    Normal log-densities of the reparameterised sample, through which a gradient flows) against
    tests/golden/tiny_gaussian_iwae.npz written by the real reference: losses, metrics, per-parameter gradient norms,
    parameters after clip + AdamW."""
    g = np.load(os.path.join(GOLD, 'tiny_gaussian_iwae.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    assert oconf.stoch_discrete == 0 and oconf.iwae_samples == 2
    model = _build(oconf, O.make_params(oconf, seed=0))
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    pre = 's0_'
    raw = {k: g[pre + 'in_' + k] for k in ('image_u8', 'action_idx', 'reward', 'terminal', 'reset')}
    noise = {k: torch.from_numpy(g[pre + 'in_' + k]).to(DEV) for k in ('u_post', 'u_act', 'u_prior', 'eps_act') if pre + 'in_' + k in g.files}
    losses, state, metrics, tensors, _ = model.training_step(_to_dev(O.preprocess(raw, oconf)),
                                                             model.init_state(oconf.batch_size * oconf.iwae_samples), noise=noise)
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
    for opt in opts:
        opt.step()
    if oconf.actor_dist == 'onehot':
        assert np.array_equal(model.last_extras['act_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_act'])
    for i, l in enumerate(losses):
        ref = g[pre + 'losses'][i]
        assert _rel(l, ref) < 2e-5 or abs(float(l) - ref) < 2e-6, (i, float(l), ref)
    for k, v in {**metrics, **gm}.items():
        ref = float(g[pre + 'metric_' + k])
        assert _rel(v, ref) < 1e-4 or abs(float(v) - ref) < 5e-6, (k, float(v), ref)
    names = [str(n) for n in g[pre + 'grad_names']]
    named = dict(model.named_parameters())
    for n, ref in zip(names, g[pre + 'grad_norms']):
        got = float(named[n].grad.double().norm())
        assert abs(got - ref) <= 2e-3 * ref + 1e-7, (n, got, ref)
    sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
    np.testing.assert_allclose(sums, g[pre + 'param_abs_sums'], rtol=2e-6)


def test_iwae_training_step_matches_reference_golden(hip):
    """SURVEY 8(f) N3 - iwae_samples = 3 (train.py:353-359,380-385 evaluate with eval_samples > 1; here as a full TRAINING
    step, gradients included) against tests/golden/tiny_iwae.npz written by the real reference: batch expansion by I
    (rssm.py:35-41), sampled KL (dreamer.py:340-343), loss_model = -logavgexp(-loss_tbi) (functions.py:97-102), two
    consecutive steps.  Bars: indices bit-exact; losses / metrics 2e-5 relative; logged tensors 2e-5; per-parameter
    gradient norms 1e-3; stored full gradients 2e-3 of their max; parameters after clip + AdamW via checksums."""
    g = np.load(os.path.join(GOLD, 'tiny_iwae.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    I = oconf.iwae_samples
    assert I == 3
    model = _build(oconf, O.make_params(oconf, seed=0))
    conf = _hip_conf(oconf)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    T, B, S = oconf.batch_length, oconf.batch_size, oconf.stoch_dim
    state = model.init_state(B * I)
    for step in range(2):
        pre = f's{step}_'
        raw = {k: g[pre + 'in_' + k] for k in ('image_u8', 'action_idx', 'reward', 'terminal', 'reset')}
        noise = {k: torch.from_numpy(g[pre + 'in_' + k]).to(DEV) for k in ('u_post', 'u_act', 'u_prior')}
        losses, state, metrics, tensors, _ = model.training_step(_to_dev(O.preprocess(raw, oconf)), state, noise=noise)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        gm = model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        assert np.array_equal(model.last_extras['post_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_post'])
        assert np.array_equal(model.last_extras['act_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_act'])
        for i, l in enumerate(losses):
            r = g[pre + 'losses'][i]
            assert _rel(l, r) < 2e-5 or abs(float(l) - r) < 2e-6, (step, i, float(l), r)
        for k, v in {**metrics, **gm}.items():
            r = float(g[pre + 'metric_' + k])
            assert _rel(v, r) < 1e-4 or abs(float(v) - r) < 2e-6, (step, k, float(v), r)
        for k, v in tensors.items():
            if k == 'image_rec':
                assert _rel(v.double().sum(), g[pre + 'tensor_image_rec_sum']) < 1e-5
                np.testing.assert_allclose(v[:1, :1].cpu().numpy(), g[pre + 'tensor_image_rec_frames'], rtol=0, atol=2e-5)
            else:
                ref = g[pre + 'tensor_' + k]
                np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=2e-5, atol=2e-5 * max(1.0, np.abs(ref).max()), err_msg=k)
        named = dict(model.named_parameters())
        for n, r in zip([str(x) for x in g[pre + 'grad_names']], g[pre + 'grad_norms']):
            got = float(named[n].grad.double().norm())
            assert abs(got - r) <= 1e-3 * r + 1e-7, (step, n, got, r)
        for key in g.files:
            if key.startswith(pre + 'grad_') and key not in (pre + 'grad_norms', pre + 'grad_names'):
                ref = g[key]
                np.testing.assert_allclose(named[key[len(pre + 'grad_'):]].grad.cpu().numpy(), ref, rtol=0,
                                           atol=2e-3 * max(np.abs(ref).max(), 1e-8), err_msg=key)
        for opt in opts:
            opt.step()
        sd = model.state_dict()
        abss = np.array([float(v.double().abs().sum()) for v in sd.values()])
        np.testing.assert_allclose(abss, g[pre + 'param_abs_sums'], rtol=2e-6)
        # step 1 runs on parameters that already differ by one AdamW update's rounding (1e-6): looser state bar there
        np.testing.assert_allclose(state[0].cpu().numpy(), g[pre + 'out_state_h'], rtol=0, atol=2e-6 if step == 0 else 1e-4)


@pytest.mark.parametrize('width,M,seed', [('tiny', 37, 5), ('tiny', 64, 5), ('tiny', 65, 5), ('tiny', 300, 5),
                                          ('mid', 37, 5), ('mid', 64, 6), ('mid', 65, 5), ('mid', 300, 13)])
def test_dream_rollout_vs_oracle(hip, width, M, seed):
    """Dreamer.dream (dreamer.py:188-216) over 5 horizon steps against the oracle, at the tiny width and at deter 256 / hidden 256 /
    stoch 8x32 (a 512-wide feature: the <= 64-row products of the cell, the actor and the heads sit on the skinny kernel there,
    at the tiny width they are tiled), for 37, 64 / 65 (the skinny kernel's one-chunk limit) and 300 rows (the whole-MLP actor
    with its gathered first layer and the action draw in its output stage: >= 256 rows).  The rollout's schedule is asserted, then
    action indices equal, features within 2e-5, reward and terminal means within 1e-4 relative + 1e-5.
    Seeds chosen on the CPU: the first of 5, 6, ... whose action and prior draws all stay >= 2e-6 from an fp32-oracle CDF edge;
    minimum distances: tiny 8.0e-5 / 4.9e-5 / 7.5e-6 / 1.6e-5, mid 3.5e-6 / 4.8e-6 (seed 6; seed 5: 2.0e-6) / 2.7e-6 / 5.7e-6
    (seed 13; seeds 5..12: 9.7e-8 .. 1.5e-6)."""
    oconf = O.tiny_conf(**(MID if width == 'mid' else {}))
    params = O.make_params(oconf)
    model = _build(oconf, params)
    Hh = 5
    g = torch.Generator().manual_seed(seed)
    h = torch.tanh(torch.randn(M, oconf.deter_dim, generator=g))
    z = F.one_hot(torch.randint(0, oconf.stoch_discrete, (M, oconf.stoch_dim), generator=g), oconf.stoch_discrete).float().reshape(M, -1)
    u_act, u_prior = torch.rand(Hh, M, generator=g), torch.rand(Hh, M, oconf.stoch_dim, generator=g)
    p = {k: v for k, v in params.items()}
    fo, ao, ro, to, xo = O.dream(p, oconf, (h, z), Hh, u_act, u_prior)
    with _record_schedules() as seen:
        fh, ah, rh, th = model.dream((h.to(DEV), z.to(DEV)), Hh, u_act=u_act.to(DEV), u_prior=u_prior.to(DEV))
    print('SCHEDULE', seen['rollout'][:1])
    big = M >= 256
    _assert_schedule(seen, rollout=dict(wzt=True, wat=True, actor_wpack=big, actor_add0=big, fuse_act=big, tw_on=False))
    assert torch.equal(ah.cpu(), ao)
    _close(fh, fo, 0, 2e-5, 'dream features')
    _close(rh.mean, ro, 1e-4, 1e-5, 'dream rewards')
    _close(th.mean, to, 1e-4, 1e-5, 'dream terminals')


def test_dream_rollout_action_draw_in_the_actor_kernel(hip):
    """Round 6: with a one-hot actor on the whole-MLP kernel (>= 256 imagined rows) the action draw of every rollout step
    (dreamer.py:198-200) happens in that kernel's output stage instead of a sampler launch.  Same rule, same operation order:
    the whole rollout - action indices, latents, features - is BIT-IDENTICAL to the run with the stand-alone sampler
    (dm_rollout_fuse_act_enable), and the action indices equal the oracle's."""
    from pydreamer_amd import hip as H
    oconf = O.tiny_conf()
    params = O.make_params(oconf, seed=3)
    model = _build(oconf, params)
    M, Hh = 300, 4
    g = torch.Generator().manual_seed(9)
    h = torch.tanh(torch.randn(M, oconf.deter_dim, generator=g))
    z = F.one_hot(torch.randint(0, oconf.stoch_discrete, (M, oconf.stoch_dim), generator=g), oconf.stoch_discrete).float().reshape(M, -1)
    u_act, u_prior = torch.rand(Hh, M, generator=g), torch.rand(Hh, M, oconf.stoch_dim, generator=g)
    fo, ao, ro, to, xo = O.dream({k: v for k, v in params.items()}, oconf, (h, z), Hh, u_act, u_prior)
    runs = []
    keep = H.lib().dm_rollout_fuse_act_enable(-1)
    try:
        for on in (1, 0):
            assert H.lib().dm_rollout_fuse_act_enable(on) == on
            fh, ah, rh, th = model.dream((h.to(DEV), z.to(DEV)), Hh, u_act=u_act.to(DEV), u_prior=u_prior.to(DEV))
            runs.append((fh.clone(), ah.clone(), rh.mean.clone(), th.mean.clone()))
    finally:
        H.lib().dm_rollout_fuse_act_enable(keep)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1].cpu(), ao), 'action draws differ from the oracle'
    _close(runs[0][0], fo, 0, 2e-5, 'dream features')


@pytest.mark.parametrize('B,T', [(6, 4), (7, 4), (50, 4), (50, 10), (7, 10)])
def test_rssm_sequence_fwd_bwd_vs_oracle(hip, B, T):
    """dm_rssm_sequence_fwd / dm_rssm_sequence_bwd stand-alone through the C-ABI at the Atari-literal cell width (deter 600,
    hidden 1000, stoch 32x32) for a 7-column data-parallel shard and the full 50 columns: at these sizes the T loop runs its
    FUSED schedule: the first step as launches (LayerNorm+ELU in the prologue of the consuming <= 64-row product, sampler in
    the epilogue of the posterior-logits product), the following steps as the LDS-weight-stationary persistent kernel
    (csrc/rssm_lds.hip; B = 6 is the shard of ranks 2-7 of an 8-way split of 50 columns).  Oracle = rssm.py:21-78,125-153,186-193 restated in fp64 (oracle.cell_forward /
    prior_head) with autograd; the loss is a random projection of (features, post, prior).
    Bars: indices identical (a uniform within 1e-6 of a CDF edge excepted: > 99.9 %), states / logits 2e-5, every parameter
    gradient and dembed within 2e-4 relative L2 (posterior indices forced to the HIP draw in the oracle).  The smallest widths
    that select each schedule, with the schedule asserted: test_gpu_rssm_schedules.py."""
    import rssm_sequence_case as RC      # the body of this test, shared with test_gpu_rssm_schedules.py
    RC.run_case(B, T, 600, 1000, 32, 32, resets=RC.resets_two, seed=11, exact_idx=False)


# ------------------------------------------------------------------------------------------- size-independent properties
def test_properties_at_atari_literal(hip):
    """BASELINE.json configs[1] (B=50,T=50,H=15,deter=600): too large for the CPU oracle inside a test, so check
    structure: finite losses, exact one-hot latents, KL >= 0, run-to-run bit determinism, and gradient accumulation
    linearity (two backward passes accumulate exactly 2x)."""
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    conf = config.atari_literal()
    torch.manual_seed(0)
    model = Dreamer(conf).to(DEV)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    oconf = O.atari_literal_conf()
    obs = _to_dev(O.preprocess(O.synthetic_batch(oconf), oconf))
    noise = _to_dev(O.make_noise(oconf))
    state = model.init_state(conf.batch_size)
    res = []
    for rep in range(2):
        model.ac.train_steps = 1     # keep critic_target fixed between the repeats
        losses, out_state, metrics, tensors, _ = model.training_step(obs, state, noise=noise)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        res.append((torch.stack([l.detach().reshape(()) for l in losses]).clone(), opts[0].flat_grad.clone(),
                    opts[2].flat_grad.clone(), model.last_extras['post_idx'].clone()))
    assert torch.isfinite(res[0][0]).all()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert torch.equal(res[0][3], res[1][3])
    z = out_state[1].view(conf.batch_size, conf.stoch_dim, conf.stoch_discrete)
    assert torch.equal(z.sum(-1), torch.ones_like(z.sum(-1))) and ((z == 0) | (z == 1)).all()
    assert (tensors['loss_kl'] >= -1e-5).all()
    assert 100 < float(metrics['loss_model']) < 2000 and torch.isfinite(opts[0].flat_grad).all()
    # accumulation: a third backward without zero_grad doubles the wm gradient exactly
    losses, *_ = model.training_step(obs, state, noise=noise)
    losses[0].backward()
    assert torch.equal(opts[0].flat_grad, 2 * res[1][1])


def test_batch_shards_sum_to_full_batch(hip):
    """Data-parallel contract on one GPU: weighted sum of per-shard gradients == full-batch gradient,
    with uniforms sliced from the global layout so every shard samples the same indices as the full batch."""
    from pydreamer_amd import dist as DP
    oconf = O.tiny_conf(batch_size=5, batch_length=4, imag_horizon=3)
    params = O.make_params(oconf, seed=2)
    T, B, S, Hh = oconf.batch_length, oconf.batch_size, oconf.stoch_dim, oconf.imag_horizon
    obs = _to_dev(O.preprocess(O.synthetic_batch(oconf), oconf))
    noise = _to_dev(O.make_noise(oconf))

    def run(ob, nz, b):
        c = O.make_conf(**{**vars(oconf), 'batch_size': b})
        m = _build(c, params)
        opts = m.init_optimizers(c.adam_lr, c.adam_lr_actor, c.adam_lr_critic, c.adam_eps)
        losses, *_ = m.training_step(ob, m.init_state(b), noise=nz)
        for loss in losses:
            loss.backward()
        return [o.flat_grad.clone() for o in opts], m.last_extras['post_idx'].clone()

    full, idx_full = run(obs, noise, B)
    acc = [torch.zeros_like(g) for g in full]
    for rank in range(2):
        ob, (lo, hi) = DP.shard_obs(obs, 2, rank)
        b = hi - lo
        nz = dict(u_post=noise['u_post'][:, lo:hi].contiguous(),
                  u_act=noise['u_act'].view(Hh, T, B)[:, :, lo:hi].reshape(Hh, -1).contiguous(),
                  u_prior=noise['u_prior'].view(Hh, T, B, S)[:, :, lo:hi].reshape(Hh, -1, S).contiguous())
        gs, idx = run(ob, nz, b)
        assert torch.equal(idx, idx_full[:, lo:hi])
        for a, g_ in zip(acc, gs):
            a += g_ * (b / B)
    for i, (a, f) in enumerate(zip(acc, full)):
        if i == 1:
            continue        # probe group: dummy^2 is batch independent
        assert _rel_l2(a, f) < 1e-4, f'group {i}'


def test_no_cpu_fallback(hip):
    """The product path must fail loudly off-device."""
    from pydreamer_amd.models import Dreamer
    oconf = O.tiny_conf()
    model = Dreamer(_hip_conf(oconf))      # parameters on CPU
    obs = O.preprocess(O.synthetic_batch(oconf), oconf)
    with pytest.raises(Exception) as e:
        model.training_step(obs, (torch.zeros(3, 64), torch.zeros(3, 64)))
    assert 'CPU' in str(e.value) or 'cuda' in str(e.value).lower()


@pytest.mark.parametrize('amp', [False, True])
def test_deferred_weight_gradients_are_bit_identical(hip, amp):
    """dm_wgrad_side_arm / _join (the decoder's weight and bias gradients on the library's side stream, beside the BPTT loop):
    same kernels, same arguments, other stream - losses, every gradient and the updated parameters are bit-identical to the
    single-stream order over three trainer iterations, fp32 and bf16 (twins of the per-layer gradient buffers)."""
    from pydreamer_amd import models as M
    oconf = O.tiny_conf(amp=amp) if amp else O.tiny_conf()
    params = O.make_params(oconf, seed=5)
    runs = []
    keep = M._WGRAD_SIDE
    try:
        for side in (False, True):
            M._WGRAD_SIDE = side
            model = _build(oconf, params)
            assert model.overlap_backward
            opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
            st = model.init_state(oconf.batch_size)
            hist = []
            for s in range(3):
                obs = _to_dev(O.preprocess(O.synthetic_batch(oconf, seed=60 + s, first=(s == 0)), oconf))
                noise = _to_dev(O.make_noise(oconf, seed=70 + s))
                losses, st2, _, _, _ = model.training_step(obs, st, noise=noise)
                for opt in opts:
                    opt.zero_grad()
                for loss in losses:
                    loss.backward()
                model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
                grads = torch.cat([o.flat_grad for o in opts]).clone()
                for opt in opts:
                    opt.step()
                st = tuple(x.clone() for x in st2)
                hist.append((([float(x) for x in losses]), grads.cpu(), torch.cat([o.flat_param for o in opts]).cpu()))
            runs.append(hist)
    finally:
        M._WGRAD_SIDE = keep
    for s, (a, b) in enumerate(zip(*runs)):
        assert a[0] == b[0], (s, a[0], b[0])
        assert torch.equal(a[1], b[1]), f'step {s}: gradients differ'
        assert torch.equal(a[2], b[2]), f'step {s}: parameters differ'
    assert float(runs[0][0][1].abs().sum()) > 0


@pytest.mark.parametrize('cfg', ['tiny', 'shard'])
def test_pipelined_ac_optimizer_is_bit_identical(hip, cfg):
    """Dreamer.pipeline_ac_optimizer: the gradient hand-over, clip and AdamW step of the actor and critic groups enqueued on the
    actor-critic stream behind their backward pass, so that the caller's stream starts the next step's forward without waiting
    for it (the four optimizer groups are independent, dreamer.py:60-71).  Same kernels, same per-stream order: losses and all
    parameters after every one of 5 trainer iterations are BIT-IDENTICAL to the serial order - the loop reads nothing between
    steps, so the next forward really is enqueued while the previous actor-critic backward is still running; the metric
    buffer (gradient norms written on the other stream) read through packed_metrics() agrees too."""
    if cfg == 'tiny':
        oconf = O.tiny_conf()
    else:      # a 7-column shard at the Atari-literal cell width: long enough streams for the overlap to be real
        oconf = O.make_conf(deter_dim=600, hidden_dim=1000, stoch_dim=32, stoch_discrete=32, cnn_depth=8, action_dim=18,
                            batch_size=7, batch_length=12, imag_horizon=5)
    params = O.make_params(oconf, seed=6)
    runs = []
    for pipelined in (False, True):
        model = _build(oconf, params)
        model.pipeline_ac_optimizer = pipelined
        opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
        st = model.init_state(oconf.batch_size)
        batches = [(_to_dev(O.preprocess(O.synthetic_batch(oconf, seed=80 + s, first=(s == 0)), oconf)),
                    _to_dev(O.make_noise(oconf, seed=90 + s))) for s in range(5)]
        hist, keep = [], []
        for s in range(5):
            obs, noise = batches[s]
            losses, st, _, _, _ = model.training_step(obs, st, noise=noise)
            for opt in opts:
                opt.zero_grad()
            for loss in losses:
                loss.backward()
            model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
            for opt in opts:
                opt.step()
            keep.append((torch.stack([l.detach().reshape(()) for l in losses]), model.metric_buffer))      # no host read inside the loop
        assert (model._opt['actor'].home is not None) == pipelined
        names, buf, idx = model.packed_metrics()
        vals = buf.tolist()
        torch.cuda.synchronize()
        runs.append(([k[0].cpu() for k in keep], torch.cat([o.flat_param for o in opts]).cpu(),
                     {n: vals[i] for n, i in zip(names, idx)}))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1], runs[1][1]), 'parameters after 5 steps differ'
    assert runs[0][2] == runs[1][2], 'last step metrics (incl. the gradient norms written on the other stream) differ'
    sd = model.state_dict()
    assert torch.isfinite(sd['ac.actor.model.0.weight']).all()


def test_early_head_window_is_bit_identical(hip):
    """The heads over the imagined states run as two row windows (ActorCritic.split_steps); in the training step the first
    one is issued on the actor-critic stream behind a progress mark of the rollout (dm_dream_rollout_marks) while the
    rollout finishes.  Same windows and kernels on another stream: losses, gradients and updated parameters are
    bit-identical to issuing both windows behind the rollout (models._HEADS_EARLY = False) and to the plain single-stream order
    (overlap_backward=False).  imag_horizon = 9: 10 imagined steps, windows [0, 6) and [6, 10)."""
    from pydreamer_amd import models as M
    oconf = O.tiny_conf(imag_horizon=9)
    assert M.ActorCritic.split_steps(10) == 6
    params = O.make_params(oconf, seed=6)
    runs = []
    keep = M._HEADS_EARLY
    try:
        for early, overlap in ((True, True), (False, True), (False, False)):
            M._HEADS_EARLY = early
            model = _build(oconf, params)
            model.overlap_backward = overlap
            opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
            st = model.init_state(oconf.batch_size)
            hist = []
            for s in range(3):
                obs = _to_dev(O.preprocess(O.synthetic_batch(oconf, seed=80 + s, first=(s == 0)), oconf))
                noise = _to_dev(O.make_noise(oconf, seed=85 + s))
                losses, st2, _, _, _ = model.training_step(obs, st, noise=noise)
                for opt in opts:
                    opt.zero_grad()
                for loss in losses:
                    loss.backward()
                model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
                grads = torch.cat([o.flat_grad for o in opts]).clone()
                for opt in opts:
                    opt.step()
                st = tuple(x.clone() for x in st2)
                hist.append(([float(x) for x in losses], grads.cpu(), torch.cat([o.flat_param for o in opts]).cpu()))
            runs.append(hist)
    finally:
        M._HEADS_EARLY = keep
    for other in runs[1:]:
        for s, (a, b) in enumerate(zip(runs[0], other)):
            assert a[0] == b[0], (s, a[0], b[0])
            assert torch.equal(a[1], b[1]), f'step {s}: gradients differ'
            assert torch.equal(a[2], b[2]), f'step {s}: parameters differ'


@pytest.mark.parametrize('amp,extra', [(False, {}), (True, {}), (False, dict(iwae_samples=3)), (False, dict(aux_critic=True))])
def test_world_model_tail_on_side_stream_is_bit_identical(hip, amp, extra):
    """The tail of the world-model forward (decoder + MSE, reward / terminal heads, KL, the loss sums, the auxiliary critic) is
    enqueued on the world-model stream in front of the pre-launched backward, with that stream's workspace, while the caller's
    stream goes from the posterior loop straight to the rollout (WorldModel._forward, Dreamer.wm_tail_on_side).  Same kernels
    on the same operands: every loss, metric, logged tensor, gradient and updated parameter equals the run with the tail on the
    caller's stream, bit for bit - fp32 and bf16, with IWAE samples, with the auxiliary critic."""
    oconf = O.tiny_conf(amp=amp, **extra)
    params = O.make_params(oconf, seed=7)
    runs = []
    for tail in (True, False):
        model = _build(oconf, params)
        model.wm_tail_on_side = tail
        opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
        st = model.init_state(oconf.batch_size * oconf.iwae_samples)
        hist = []
        for s in range(3):
            obs = _to_dev(O.preprocess(O.synthetic_batch(oconf, seed=90 + s, first=(s == 0)), oconf))
            torch.manual_seed(95 + s)              # the samplers' uniforms come from torch's generator: same draws in both runs
            losses, st2, metrics, tensors, _ = model.training_step(obs, st)
            assert (model.wm._last_pack.get('tail') is not None) == tail
            for opt in opts:
                opt.zero_grad()
            for loss in losses:
                loss.backward()
            model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
            grads = torch.cat([o.flat_grad for o in opts]).clone()
            for opt in opts:
                opt.step()
            st = tuple(x.clone() for x in st2)
            hist.append(([float(x) for x in losses], {k: float(v) for k, v in metrics.items()},
                         {k: v.detach().float().cpu() for k, v in tensors.items()}, grads.cpu(),
                         torch.cat([o.flat_param for o in opts]).cpu()))
        runs.append(hist)
    for s, (a, b) in enumerate(zip(*runs)):
        assert a[0] == b[0], (s, a[0], b[0])
        assert a[1] == b[1], (s, {k: (a[1][k], b[1][k]) for k in a[1] if a[1][k] != b[1][k]})
        assert a[2].keys() == b[2].keys()
        for k in a[2]:
            assert torch.equal(a[2][k], b[2][k]), f'step {s}: tensor {k} differs'
        assert torch.equal(a[3], b[3]), f'step {s}: gradients differ'
        assert torch.equal(a[4], b[4]), f'step {s}: parameters differ'


@pytest.mark.parametrize('extra', [dict(), dict(target_interval=10), dict(actor_dist='tanh_normal', action_dim=4, entropy=1.0e-4),
                                   dict(stoch_discrete=0, stoch_dim=16), dict(gru_type='gru_layernorm', gru_layers=2, deter_dim=64),
                                   dict(aux_critic=True, target_interval_aux=7, target_interval=9)],
                         ids=['default', 'target_refresh', 'continuous_actor', 'gaussian_latents', 'layernorm_gru_stack', 'aux_critic'])
def test_forty_trainer_iterations_on_a_fixed_batch_learn_like_the_oracle(hip, extra):
    """The whole trainer section (train.py:165-198: training_step, zero_grad, four backward passes, grad_clip, four AdamW steps) run
    FORTY times on one fixed batch from the same initial parameters, on the oracle (CPU, torch.optim.AdamW) and on this build
    (flat-buffer AdamW, side streams, buffer-swap gradient hand-over in its steady state): the world-model loss must FALL on both
    (522 -> 482 on the oracle; variants: critic-target refreshes inside the window, a continuous actor, Gaussian latents, a two-layer
    LayerNorm GRU stack, the auxiliary critic with its own target interval) and the two trajectories must stay together - parameters that have gone through 40 optimizer steps of
    this build give the loss the reference's arithmetic gives, to 1e-4 relative at every step (measured on MI355X: worst gap 2.4e-7,
    522.278 -> 482.429 on both)."""
    oconf = O.tiny_conf(adam_lr=1e-3, adam_lr_actor=3e-4, adam_lr_critic=3e-4, **extra)
    params = O.make_params(oconf, seed=3)
    ora = O.OracleDreamer(oconf, params)
    ora.init_optimizers()
    model = _build(oconf, params)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    obs = O.preprocess(O.synthetic_batch(oconf, seed=1234, first=True), oconf)
    obs_d = _to_dev(obs)
    n_iter = 40 if not extra else 20          # (the variants run half the window: ~0.7 s per iteration on the box, mostly host)
    traj_o, traj_h, worst = [], [], 0.0
    for s in range(n_iter):
        noise = O.make_noise(oconf, seed=777 + s)
        lo, _, mo, _, _ = ora.training_step(obs, ora.init_state(oconf.batch_size), noise)
        ora.backward_clip_step(lo)
        lh, _, mh, _, _ = model.training_step(obs_d, model.init_state(oconf.batch_size), noise=_to_dev(noise))
        for opt in opts:
            opt.zero_grad()
        for loss in lh:
            loss.backward()
        model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        for opt in opts:
            opt.step()
        a, b = float(lh[0]), float(lo[0])
        assert np.isfinite(a) and all(np.isfinite(float(x)) for x in lh), (s, [float(x) for x in lh])
        worst = max(worst, abs(a - b) / abs(b))
        assert abs(a - b) / abs(b) < 1e-4, (s, a, b)
        traj_o.append(b)
        traj_h.append(a)
    print(f'fixed-batch training: oracle {traj_o[0]:.3f} -> {traj_o[-1]:.3f}, build {traj_h[0]:.3f} -> {traj_h[-1]:.3f}, worst relative gap {worst:.2e}')
    assert traj_h[-1] < (0.95 if n_iter == 40 else 0.985) * traj_h[0] and traj_o[-1] < (0.95 if n_iter == 40 else 0.985) * traj_o[0]
    assert all(traj_h[i + 5] < traj_h[i] for i in range(0, n_iter - 5, 5)), traj_h      # falling over every 5-step window
    # the replicas after 40 steps: parameters of the two implementations, group by group
    sd = model.state_dict()
    for k, v in ora.p.items():
        if O.group_of(k) is None or k not in sd:
            continue
        e = float((sd[k].detach().cpu().double() - v.detach().double()).norm() / (v.detach().double().norm() + 1e-12))
        assert e < 5e-3, (k, e)


def _prove_imagination_divergences(fixture, model, oconf, g, noise, max_rows=8, edge=1e-6):
    """Every imagined trajectory (column r of the (H, M) rollout) either draws EXACTLY the reference's action and latent indices
    at all H steps, or its FIRST differing draw - in the reference's call order: per step the actor's draw (dreamer.py:198-200),
    then the prior's 32 latent draws (rssm.py:177-179) - is proven to sit on a CDF edge: the softmax / cumsum of THIS build's own
    logits is recomputed in fp64 (actor logits as the rollout kept them; prior logits from the build's own h_{i+1} =
    dream_features[i+1, r, :D] through the oracle's prior head in fp64) and the draw's uniform must lie within `edge` of the
    boundary between the two classes (fp32 logits summed in another order than torch's CPU kernels move a boundary by ~1e-7;
    measured on MI355X, profiles/r06_parity_margins.txt: atari_literal 3 of 2 500 trajectories, worst margin 1.0e-7; dmc_native 5,
    1.2e-7; atari_native none - the bar is 10x that).
    Every draw BEFORE that one equals the reference's by construction of "first"; a trajectory that has left the reference's
    carries another state afterwards, so its later draws are not comparable.  No trajectory passes without a measured margin.
    Returns the records (also printed: scripts/parity_margins.sh collects them into profiles/)."""
    act = model.last_extras['act_idx'].cpu().numpy().astype(np.int64)
    Hh, M = act.shape
    D_, S_, C_ = oconf.deter_dim, oconf.stoch_dim, oconf.stoch_discrete
    feats = model.last_extras['dream_features']
    lat = feats[1:, :, D_:].reshape(Hh, M, S_, C_).argmax(-1).cpu().numpy().astype(np.int64)   # latent drawn at step i = z of state i+1
    ref_lat = g['s0_idx_lat'].astype(np.int64)
    assert ref_lat.shape == lat.shape, 'fixture holds the full (H, M, S) latent index tensor (oracle/gen_golden.py)'
    onehot = oconf.actor_dist == 'onehot'
    ref_act = g['s0_idx_act'].astype(np.int64) if onehot else act
    act_same, lat_same = act == ref_act, lat == ref_lat
    print(f'{fixture}: imagination actor indices equal: {act_same.mean():.6f}, latent indices equal: {lat_same.mean():.6f}')
    rows = np.flatnonzero(~(act_same.all(axis=0) & lat_same.all(axis=(0, 2))))
    records = []
    if len(rows):
        p64 = {k: v.double() for k, v in O.make_params(oconf, seed=0).items() if k.startswith('wm.core.cell.prior')}
        logits_a = model.last_extras['actor_logits'].view(Hh, M, -1).double().cpu() if onehot else None
    for r in rows:
        ha = int(np.argmax(~act_same[:, r])) if not act_same[:, r].all() else Hh
        hl = int(np.argmax(~lat_same[:, r].all(axis=-1))) if not lat_same[:, r].all() else Hh
        if ha <= hl:            # the action draw of step ha comes before the latent draws of step ha
            assert lat_same[:ha, r].all() and act_same[:ha, r].all()
            cdf = torch.softmax(logits_a[ha, r], -1).cumsum(-1)
            lo, hi = sorted((int(act[ha, r]), int(ref_act[ha, r])))
            margin = float((cdf[lo:hi] - float(noise['u_act'][ha, r]) * cdf[-1]).abs().min())
            records.append(('action', int(r), ha, -1, margin))
        else:
            assert lat_same[:hl, r].all() and act_same[:hl + 1, r].all()
            h_next = feats[hl + 1, r, :D_].double().cpu()
            pl = O.prior_head(p64, h_next[None])[0].view(S_, C_)
            cdf = torch.softmax(pl, -1).cumsum(-1)
            for s_ in np.flatnonzero(~lat_same[hl, r]):      # every group that flipped in that draw call stands on its own
                lo, hi = sorted((int(lat[hl, r, s_]), int(ref_lat[hl, r, s_])))
                margin = float((cdf[s_, lo:hi] - float(noise['u_prior'][hl, r, s_]) * cdf[s_, -1]).abs().min())
                records.append(('latent', int(r), hl, int(s_), margin))
    for kind, r, h, s_, margin in records:
        print(f'  trajectory {r}: first divergence at step {h}, {kind} draw' + (f' group {s_}' if s_ >= 0 else '') +
              f', |cdf edge - u cdf_last| = {margin:.3e}')
        assert margin < edge, f'{fixture}: trajectory {r} diverges at {kind} step {h} away from a CDF edge (margin {margin:.3e})'
    print(f'{fixture}: {len(rows)} of {M} imagined trajectories diverge, every one at a proven CDF edge '
          f'(worst margin {max([x[4] for x in records], default=0.0):.3e})')
    assert len(rows) <= max_rows
    return records



@pytest.mark.parametrize('fixture', ['atari_literal', 'atari_native'])
def test_training_step_matches_reference_at_atari_literal(hip, fixture):
    """BASELINE.json configs[1] at FULL size against the slim golden written by the real reference
    (tests/golden/atari_literal.npz; inputs regenerated from the same seeds and fingerprinted), and the same replay at
    pydreamer's OWN shipped Atari configuration (tests/golden/atari_native.npz: defaults+atari, B=32, T=48, deter_dim 1024 -
    config/defaults.yaml:49-50,198; what README.md:90-97 measured and `bench.py --workload atari-native` runs).
    117 500 categorical draws depend on fp32 logits summed in a different order than torch's CPU kernels, so a draw whose
    uniform lies within ~1 ulp of a CDF edge may legitimately differ and then changes that row's later states; the bar is
    therefore: every index of the first 25 time steps identical, >= 99.99 % of all posterior indices identical, loss_model
    within 1e-3 absolute, the other losses within 1e-3 relative, per-parameter gradient norms within 3e-3 and gradient
    projections within 5e-3 of the parameter's gradient norm (bars ~10x the measured values).  Measured on MI355X (round 1): all 80 000 posterior
    indices identical, loss_model 523.5302124 = reference to the last printed digit, loss_actor 2e-4 / loss_critic 3e-5
    relative, worst per-parameter gradient-norm error 3.1e-4."""
    g = np.load(os.path.join(GOLD, fixture + '.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    if fixture == 'atari_native':
        assert (oconf.batch_size, oconf.batch_length, oconf.deter_dim, oconf.imag_horizon) == (32, 48, 1024, 15)
    raw = O.synthetic_batch(oconf, seed=1234, first=True)
    noise = O.make_noise(oconf, seed=777)
    assert int(raw['image_u8'].astype(np.int64).sum()) == int(g['s0_in_image_sum']), 'input generator drifted'
    model = _build(oconf, O.make_params(oconf, seed=0))
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    losses, state, metrics, tensors, _ = model.training_step(_to_dev(O.preprocess(raw, oconf)),
                                                             model.init_state(oconf.batch_size), noise=_to_dev(noise))
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
    got = model.last_extras['post_idx'].cpu().numpy().astype(np.uint8)
    ref = g['s0_idx_post']
    same = (got == ref)
    print(fixture, 'posterior indices equal:', same.mean(), 'first mismatch t:',
          int(np.argmax(~same.all(axis=(1, 2)))) if not same.all() else None)
    # every posterior index of the full-size step equals the reference's (measured 100 % in every round; an ulp-edge escape
    # would be added here only with a measured mismatch to justify it)
    assert same.all(), f'{int((~same).sum())} of {same.size} posterior indices differ from the reference'
    # imagination indices (dreamer.py:194-205, rssm.py:155-184): EXACT - or PROVEN to sit on a CDF edge, trajectory by trajectory
    _prove_imagination_divergences(fixture, model, oconf, g, noise)
    # the north-star bar: world-model loss within 1e-3 (absolute) of the reference on the fixed full-size batch
    assert abs(float(losses[0]) - g['s0_losses'][0]) < 1e-3
    for i, l in enumerate(losses):
        r = g['s0_losses'][i]
        print('loss', i, float(l), r)
        assert _rel(l, r) < 1e-3 or abs(float(l) - r) < 1e-4, (i, float(l), r)
    for k, v in {**metrics, **gm}.items():
        r = float(g['s0_metric_' + k])
        assert _rel(v, r) < 5e-3 or abs(float(v) - r) < 1e-4, (k, float(v), r)
    names = [str(n) for n in g['s0_grad_names']]
    named = dict(model.named_parameters())
    worst = max(abs(float(named[n].grad.double().norm()) - r) / max(r, 1e-7) for n, r in zip(names, g['s0_grad_norms']))
    print('worst per-parameter grad-norm rel err', worst)
    assert worst < 3e-3          # measured 3.1e-4 (Atari-literal) / 9.3e-4 (DMC-native)
    if 's0_grad_proj' in g.files:      # gradient DIRECTIONS: projections onto two closed-form directions per parameter
        wp = 0.0
        for i, (n, r, pr) in enumerate(zip(names, g['s0_grad_norms'], g['s0_grad_proj'])):
            got = O.grad_probe(named[n].grad, i)
            wp = max(wp, max(abs(got[0] - pr[0]), abs(got[1] - pr[1])) / max(r, 1e-7))
        print('worst per-parameter gradient-projection error / norm', wp)
        assert wp < 5e-3         # measured 2.7e-3 / 1.8e-3


def test_training_step_matches_reference_at_dmc_native(hip):
    """BASELINE.json configs[4] at its native width - defaults+dmc (deter_dim 2048, hidden 1000, tanh_normal actor on 6
    continuous action dims, actor_grad=reinforce) at B=50, T=50, H=15, fp32 - against the slim golden written by the real
    reference (tests/golden/dmc_native.npz).  Bars as for Atari-literal: first 25 time steps of posterior indices
    identical, >= 99.99 % overall, loss_model within 1e-3 absolute, other losses / metrics within 1e-3 .. 5e-3 relative,
    per-parameter gradient norms within 3e-3, gradient projections within 5e-3."""
    g = np.load(os.path.join(GOLD, 'dmc_native.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    assert oconf.deter_dim == 2048 and oconf.actor_dist == 'tanh_normal' and oconf.action_dim == 6
    raw = O.synthetic_batch(oconf, seed=1234, first=True)
    noise = O.make_noise(oconf, seed=777)
    assert int(raw['image_u8'].astype(np.int64).sum()) == int(g['s0_in_image_sum']), 'input generator drifted'
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    conf = config.load_config('defaults', 'dmc', **{k: getattr(oconf, k) for k in vars(oconf)})
    model = Dreamer(conf)
    model.load_state_dict(O.make_params(oconf, seed=0), strict=True)
    model = model.to(DEV)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    losses, state, metrics, tensors, _ = model.training_step(_to_dev(O.preprocess(raw, oconf)),
                                                             model.init_state(oconf.batch_size), noise=_to_dev(noise))
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
    same = model.last_extras['post_idx'].cpu().numpy().astype(np.uint8) == g['s0_idx_post']
    print('dmc-native posterior indices equal:', same.mean())
    assert same[:25].all() and same.mean() >= 0.9999
    if same.all():      # imagined latents are comparable only from the reference's own start states
        _prove_imagination_divergences('dmc_native', model, oconf, g, noise)
    assert abs(float(losses[0]) - g['s0_losses'][0]) < 1e-3
    for i, l in enumerate(losses):
        r = g['s0_losses'][i]
        print('loss', i, float(l), r)
        assert _rel(l, r) < 2e-3 or abs(float(l) - r) < 2e-4, (i, float(l), r)
    for k, v in {**metrics, **gm}.items():
        r = float(g['s0_metric_' + k])
        assert _rel(v, r) < 5e-3 or abs(float(v) - r) < 2e-4, (k, float(v), r)
    names = [str(n) for n in g['s0_grad_names']]
    named = dict(model.named_parameters())
    worst = max(abs(float(named[n].grad.double().norm()) - r) / max(r, 1e-7) for n, r in zip(names, g['s0_grad_norms']))
    print('worst per-parameter grad-norm rel err', worst)
    assert worst < 3e-3          # measured 3.1e-4 (Atari-literal) / 9.3e-4 (DMC-native)
    if 's0_grad_proj' in g.files:      # gradient DIRECTIONS: projections onto two closed-form directions per parameter
        wp = 0.0
        for i, (n, r, pr) in enumerate(zip(names, g['s0_grad_norms'], g['s0_grad_proj'])):
            got = O.grad_probe(named[n].grad, i)
            wp = max(wp, max(abs(got[0] - pr[0]), abs(got[1] - pr[1])) / max(r, 1e-7))
        print('worst per-parameter gradient-projection error / norm', wp)
        assert wp < 5e-3         # measured 2.7e-3 / 1.8e-3


def test_dmc_native_bf16_step_tracks_the_fp32_reference(hip):
    """BASELINE.json configs[4] as named: DMC continuous actions (deter 2048, tanh_normal, action_dim 6) at B=50, T=50, H=15
    WITH mixed precision (conf.amp: bf16 MFMA operands, every bf16 kernel variant of this size: tiled GEMMs, row panels,
    whole-MLP kernel), backward and optimizer step included.  The forward is pinned on the reference's own autocast run by
    test_amp_against_reference_autocast_golden[dmc_native_amp]; autocast gradients are not stored (several minutes of CPU per
    backward at this width), so the GRADIENT pin here is the fp32 reference fixture at a bf16-class bar with the posterior
    indices forced to the reference's: loss_model within 2e-3 relative, per-parameter world-model gradient norms within 5e-2,
    everything finite; plus a full optimizer step."""
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    g = np.load(os.path.join(GOLD, 'dmc_native.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    raw = O.synthetic_batch(oconf, seed=1234, first=True)
    noise = O.make_noise(oconf, seed=777)
    conf = config.load_config('defaults', 'dmc', **{**{k: getattr(oconf, k) for k in vars(oconf)}, 'amp': True})
    model = Dreamer(conf)
    model.load_state_dict(O.make_params(oconf, seed=0), strict=True)
    model = model.to(DEV)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    fidx = torch.from_numpy(g['s0_idx_post'].astype(np.int64)).to(DEV)
    losses, state, metrics, tensors, _ = model.training_step(_to_dev(O.preprocess(raw, oconf)), model.init_state(oconf.batch_size),
                                                             noise=_to_dev(noise), forced_idx=fidx)
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
    for opt in opts:
        opt.step()
    print('dmc bf16 loss_model', float(losses[0]), 'fp32 reference', float(g['s0_losses'][0]))
    assert all(bool(torch.isfinite(l)) for l in losses) and all(bool(torch.isfinite(v)) for v in gm.values())
    assert _rel(losses[0], g['s0_losses'][0]) < 2e-3
    names = [str(n) for n in g['s0_grad_names']]
    named = dict(model.named_parameters())
    worst = max(abs(float(named[n].grad.double().norm()) - r) / max(r, 1e-7)
                for n, r in zip(names, g['s0_grad_norms']) if n.startswith('wm.'))
    print('worst world-model grad-norm rel err under bf16 operands', worst)
    assert worst < 5e-2
    assert all(bool(torch.isfinite(o.flat_param).all()) for o in opts)


def test_uint8_ingest_matches_float_path(hip):
    """training_step consumes the replay's native uint8 (T,B,H,W,C) frames directly - x/255-0.5 and
    HWC->CHW (preprocessing.py:21-29) happen inside the first conv's patch loader and inside the MSE kernel, no float image
    is written.  The whole step (losses, reconstruction, every gradient) is bit-identical to the float path; and the
    stand-alone dm_preprocess_image_u8 primitive equals the host-side preprocessing bit for bit."""
    import ctypes
    oconf = O.tiny_conf()
    raw = O.synthetic_batch(oconf, seed=21, first=True)
    obs_f = _to_dev(O.preprocess(raw, oconf))
    u8 = torch.from_numpy(raw['image_u8']).to(DEV)
    obs_u = dict(obs_f, image=u8)
    noise = _to_dev(O.make_noise(oconf, seed=22))
    outs = []
    for obs in (obs_f, obs_u):
        model = _build(oconf, O.make_params(oconf, seed=2))
        model.overlap_backward = False
        conf = _hip_conf(oconf)
        opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
        losses, st, metrics, tensors, _ = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        outs.append(([float(x) for x in losses], tensors['image_rec'].cpu(), opts[0].flat_grad.clone().cpu(),
                     model.wm._last_pack['image'].dtype))
    assert outs[0][3] == torch.float32 and outs[1][3] == torch.uint8          # the uint8 frames were consumed as they are
    assert outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][2], outs[1][2])
    T, B = u8.shape[:2]
    dst = torch.empty(T, B, 3, 64, 64, device=DEV)
    hip.call('dm_preprocess_image_u8', T * B, 64 * 64, 3, hip.ptr(u8), hip.fptr(dst), hip.stream())
    assert torch.equal(dst, obs_f['image'])


@pytest.mark.parametrize('name', ['tiny_eval', 'tiny_eval_iwae'])
def test_logging_variants_match_reference_golden(hip, name):
    """do_image_pred + do_dream_tensors (dreamer.py:163-180,381-394) through the HIP path against
    tests/golden/tiny_eval.npz written by the real reference (called under no_grad like train.py:353-359).
    tiny_eval_iwae: evaluate()'s own call shape - iwae_samples=3 passed together with the flags (train.py:380-385)."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    Ie = int(g['iwae_samples']) if 'iwae_samples' in g.files else None
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    raw = {k: g['in_' + k] for k in ('image_u8', 'action_idx', 'reward', 'terminal', 'reset')}
    noise = {k[3:]: torch.from_numpy(g[k]).to(DEV) for k in g.files if k.startswith('in_u_') or k.startswith('in_eps_')}
    model = _build(oconf, O.make_params(oconf, seed=0))
    with torch.no_grad():
        losses, st, metrics, tensors, dt = model.training_step(_to_dev(O.preprocess(raw, oconf)),
                                                               model.init_state(oconf.batch_size * (Ie or 1)), noise=noise,
                                                               iwae_samples=Ie, do_image_pred=True, do_dream_tensors=True)
    T, B, S = oconf.batch_length, oconf.batch_size * (Ie or 1), oconf.stoch_dim
    assert np.array_equal(model.last_extras['post_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_post'])
    assert np.array_equal(model.last_extras['pred_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_pred'])
    assert np.array_equal(model.last_extras['dream_log_act_idx'].cpu().numpy().astype(np.uint8), g['idx_log_act'])
    for i, l in enumerate(losses):
        assert _rel(l, g['losses'][i]) < 2e-5 or abs(float(l) - g['losses'][i]) < 2e-6
    for k in [f[7:] for f in g.files if f.startswith('metric_')]:
        ref = float(g['metric_' + k])
        if np.isnan(ref):
            assert torch.isnan(metrics[k]), k
        else:
            assert _rel(metrics[k], ref) < 1e-4 or abs(float(metrics[k]) - ref) < 5e-6, (k, float(metrics[k]), ref)
    for k in [f[7:] for f in g.files if f.startswith('tensor_') and not f.endswith(('_sum', '_frame'))]:
        np.testing.assert_allclose(tensors[k].cpu().numpy(), g['tensor_' + k], rtol=1e-4, atol=2e-5, equal_nan=True, err_msg=k)
    assert _rel(tensors['image_pred'].double().sum(), g['tensor_image_pred_sum']) < 1e-5
    np.testing.assert_allclose(tensors['image_pred'][:1, :1].cpu().numpy(), g['tensor_image_pred_frame'], rtol=0, atol=3e-5)
    for k in [f[6:] for f in g.files if f.startswith('dream_') and not f.startswith('dream_image_pred')]:
        np.testing.assert_allclose(dt[k].cpu().numpy(), g['dream_' + k], rtol=1e-4, atol=2e-5, err_msg=k)
    assert _rel(dt['image_pred'].double().sum(), g['dream_image_pred_sum']) < 1e-5
    np.testing.assert_allclose(dt['image_pred'][-1:, :1].cpu().numpy(), g['dream_image_pred_frame'], rtol=0, atol=3e-5)


@pytest.mark.parametrize('name', ['tiny_open_loop', 'tiny_open_loop_iwae'])
def test_open_loop_matches_reference_golden(hip, name):
    """do_open_loop (rssm.py:50-53: every step is forward_prior) + the logging variants, against
    tests/golden/tiny_open_loop.npz written by the real reference; evaluation only (no_grad).
    tiny_open_loop_iwae: with iwae_samples=3, the call of train.py:353-359."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    Ie = int(g['iwae_samples']) if 'iwae_samples' in g.files else None
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    raw = {k: g['in_' + k] for k in ('image_u8', 'action_idx', 'reward', 'terminal', 'reset')}
    noise = {k[3:]: torch.from_numpy(g[k]).to(DEV) for k in g.files if k.startswith('in_u_') or k.startswith('in_eps_')}
    model = _build(oconf, O.make_params(oconf, seed=0))
    obs = _to_dev(O.preprocess(raw, oconf))
    with pytest.raises(NotImplementedError):
        model.training_step(obs, model.init_state(oconf.batch_size * (Ie or 1)), noise=noise, iwae_samples=Ie, do_open_loop=True)
    with torch.no_grad():
        losses, st, metrics, tensors, dt = model.training_step(obs, model.init_state(oconf.batch_size * (Ie or 1)), noise=noise,
                                                               iwae_samples=Ie, do_image_pred=True, do_dream_tensors=True,
                                                               do_open_loop=True)
    T, B, S = oconf.batch_length, oconf.batch_size * (Ie or 1), oconf.stoch_dim
    assert np.array_equal(model.last_extras['post_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_post'])
    assert np.array_equal(model.last_extras['pred_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_pred'])
    np.testing.assert_allclose(st[0].cpu().numpy(), g['out_state_h'], rtol=0, atol=5e-6)
    for i, l in enumerate(losses):
        assert _rel(l, g['losses'][i]) < 2e-5 or abs(float(l) - g['losses'][i]) < 2e-6, (i, float(l), g['losses'][i])
    for k in [f[7:] for f in g.files if f.startswith('metric_')]:
        ref = float(g['metric_' + k])
        if np.isnan(ref):
            assert torch.isnan(metrics[k]), k
        else:
            assert _rel(metrics[k], ref) < 1e-4 or abs(float(metrics[k]) - ref) < 5e-6, (k, float(metrics[k]), ref)
    for k in [f[7:] for f in g.files if f.startswith('tensor_') and not f.endswith(('_sum', '_frame'))]:
        np.testing.assert_allclose(tensors[k].cpu().numpy(), g['tensor_' + k], rtol=1e-4, atol=2e-5, equal_nan=True, err_msg=k)
    for k in [f[6:] for f in g.files if f.startswith('dream_') and not f.startswith('dream_image_pred')]:
        np.testing.assert_allclose(dt[k].cpu().numpy(), g['dream_' + k], rtol=1e-4, atol=2e-5, err_msg=k)


@pytest.mark.parametrize('amp', [False, True])
def test_literal_trainer_section(hip, amp):
    """BASELINE north-star: "train.py drives it unchanged".  The statement sequence of train.py:165-198, verbatim in structure
    - autocast(enabled=conf.amp) around training_step, GradScaler(enabled=conf.amp), zero_grad x4, scaler.scale(loss).backward()
    x4, scaler.unscale_(opt) x4, model.grad_clip, scaler.step(opt) x4, scaler.update() - against the plain sequence
    (backward / clip / step) on an identical model, for amp False and True.  Two steps with carried state: every parameter
    identical bit for bit (a disabled scaler is a pass-through; an enabled one multiplies the four losses by 2^16 and the
    gradients by 2^-16, both exact in fp32).  Then, amp only, an overflow step: an inf planted in one world-model gradient
    makes scaler.step skip THAT optimizer (its parameters and moments stay put), the others step, and update() halves the scale."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from torch.cuda.amp import GradScaler, autocast
    oconf = O.tiny_conf()
    conf = _hip_conf(oconf)
    conf.amp = amp
    params = O.make_params(oconf, seed=6)
    from pydreamer_amd.models import Dreamer

    def build():
        m = Dreamer(conf)
        m.load_state_dict(params, strict=True)
        m = m.to(DEV)
        return m, m.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    batches = [_to_dev(O.preprocess(O.synthetic_batch(oconf, seed=70 + i, first=(i == 0)), oconf)) for i in range(3)]
    noises = [{k: v.to(DEV) for k, v in O.make_noise(oconf, seed=80 + i).items()} for i in range(3)]

    model, optimizers = build()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        scaler = GradScaler(enabled=conf.amp)
    states, wid = {}, 0
    for i in range(2):                                   # ---- train.py:165-198
        obs = batches[i]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ctx = autocast(enabled=conf.amp)
        with ctx:
            state = states.get(wid)
            if state is None:
                state = model.init_state(conf.batch_size * conf.iwae_samples)
            losses, new_state, loss_metrics, tensors, dream_tensors = \
                model.training_step(obs, state, do_image_pred=(i == 1), do_dream_tensors=(i == 1), noise=noises[i])
            if conf.keep_state:
                states[wid] = new_state
        for opt in optimizers:
            opt.zero_grad()
        for loss in losses:
            scaler.scale(loss).backward()
        for opt in optimizers:
            scaler.unscale_(opt)
        grad_metrics = model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for opt in optimizers:
            scaler.step(opt)
        scaler.update()
        assert all(np.isfinite(v.item()) for v in grad_metrics.values())
        assert i == 0 or ('image_pred' in tensors and 'image_pred' in dream_tensors)

    plain, popts = build()
    st = plain.init_state(conf.batch_size)
    for i in range(2):
        losses_p, st, _, _, _ = plain.training_step(batches[i], st, do_image_pred=(i == 1), do_dream_tensors=(i == 1), noise=noises[i])
        for opt in popts:
            opt.zero_grad()
        for loss in losses_p:
            loss.backward()
        gm_p = plain.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for opt in popts:
            opt.step()
    for (k, a), (_, b) in zip(model.state_dict().items(), plain.state_dict().items()):
        assert torch.equal(a, b), k
    for k in gm_p:
        assert torch.equal(grad_metrics[k], gm_p[k]), k
    for a, b in zip(losses, losses_p):
        assert torch.equal(a.detach(), b.detach())

    if not amp:
        assert scaler.get_scale() == 1.0
        return
    # ---- overflow step: GradScaler must skip the optimizer whose gradients hold an inf, and only that one
    scale0 = scaler.get_scale()
    before = [o.flat_param.clone() for o in optimizers]
    moments = optimizers[0].exp_avg.clone()
    with autocast(enabled=True):
        losses, new_state, *_ = model.training_step(batches[2], states[wid], noise=noises[2])
    for opt in optimizers:
        opt.zero_grad()
    for loss in losses:
        scaler.scale(loss).backward()
    model.wm.core.cell.z_mlp.weight.grad.view(-1)[3] = float('inf')
    for opt in optimizers:
        scaler.unscale_(opt)
    model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
    for opt in optimizers:
        scaler.step(opt)
    scaler.update()
    assert torch.equal(optimizers[0].flat_param, before[0]) and torch.equal(optimizers[0].exp_avg, moments)      # wm: skipped
    assert not torch.equal(optimizers[2].flat_param, before[2]) and not torch.equal(optimizers[3].flat_param, before[3])
    assert scaler.get_scale() == scale0 * 0.5


def test_backward_of_an_older_step_is_valid(hip):
    """Every training_step() owns its buffers (the per-geometry arena of the chains' hipGraph replay is gone with the replay):
    with overlap_backward off (gradients computed inside backward()) the losses of an OLDER step can still be backpropagated
    after a newer step ran, and give that older step's gradients."""
    oconf = O.tiny_conf()
    model = _build(oconf, O.make_params(oconf, seed=1))
    model.overlap_backward = False
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    obs = _to_dev(O.preprocess(O.synthetic_batch(oconf, seed=3, first=True), oconf))
    obs2 = _to_dev(O.preprocess(O.synthetic_batch(oconf, seed=4, first=True), oconf))
    noise = _to_dev(O.make_noise(oconf, seed=5))
    st = model.init_state(oconf.batch_size)
    losses1, *_ = model.training_step(obs, st, noise=noise)
    for opt in opts:
        opt.zero_grad()
    losses1[0].backward()
    want = opts[0].flat_grad.clone()
    losses1, *_ = model.training_step(obs, st, noise=noise)
    losses2, *_ = model.training_step(obs2, st, noise=noise)
    for opt in opts:
        opt.zero_grad()
    losses1[0].backward()
    assert torch.equal(opts[0].flat_grad, want)
    for opt in opts:
        opt.zero_grad()
    for loss in losses2:
        loss.backward()
    assert not torch.equal(opts[0].flat_grad, want)

def test_stale_prelaunched_gradients_are_refused(hip):
    """Pre-launched backward passes write into a per-optimizer scratch buffer; a backward() on losses of an OLDER
    training_step() (its scratch was overwritten) must fail loudly instead of delivering the wrong gradients."""
    oconf = O.tiny_conf()
    model = _build(oconf, O.make_params(oconf, seed=1))
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    obs = _to_dev(O.preprocess(O.synthetic_batch(oconf, seed=3, first=True), oconf))
    st = model.init_state(oconf.batch_size)
    losses1, *_ = model.training_step(obs, st)
    losses2, *_ = model.training_step(obs, st)
    for opt in opts:
        opt.zero_grad()
    with pytest.raises(RuntimeError, match='overwritten'):
        losses1[0].backward()
    for loss in losses2:
        loss.backward()


def test_amp_bf16_step_tracks_fp32(hip):
    """conf.amp=True (BASELINE configs[2]): every tiled GEMM takes bf16 operands with fp32 accumulation.  The step must
    stay close to the fp32 oracle (bf16 has an 8-bit mantissa: 4e-3 per operand, averaged over K), be deterministic, and
    really differ from the fp32 path.  Bars measured on MI355X: losses within 2e-2 relative, world-model gradient
    direction cosine > 0.999."""
    oconf = O.tiny_conf()
    params = O.make_params(oconf, seed=4)
    obs_c = O.preprocess(O.synthetic_batch(oconf, seed=31, first=True), oconf)
    noise_c = O.make_noise(oconf, seed=32)
    ora = O.OracleDreamer(oconf, params)
    ora.init_optimizers()
    lo, _, mo, _, xo = ora.training_step(obs_c, ora.init_state(oconf.batch_size), noise_c)
    _, go = ora.backward_clip_step(lo)
    fidx = xo['post_idx'].reshape(oconf.batch_length, oconf.batch_size, -1).to(DEV)
    runs = []
    try:
        for amp in (True, True, False):
            from pydreamer_amd import config
            conf = config.load_config('defaults', 'atari', **{**{k: getattr(oconf, k) for k in vars(oconf)}, 'amp': amp})
            from pydreamer_amd.models import Dreamer
            model = Dreamer(conf)
            model.load_state_dict(params, strict=True)
            model = model.to(DEV)
            opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
            losses, st, metrics, _, _ = model.training_step(_to_dev(obs_c), model.init_state(oconf.batch_size),
                                                            noise=_to_dev(noise_c), forced_idx=fidx)
            for opt in opts:
                opt.zero_grad()
            for loss in losses:
                loss.backward()
            runs.append(([float(x) for x in losses], opts[0].flat_grad.clone(), model))
    finally:
        pass        # precision is a per-call argument: nothing to restore
    (l1, g1, m1), (l2, g2, _), (l3, g3, _) = runs
    assert l1 == l2 and torch.equal(g1, g2), 'bf16 path is not deterministic'
    assert l1 != l3, 'amp=True did not change the arithmetic'
    assert abs(l1[0] - float(lo[0])) < 2e-2 * abs(float(lo[0]))
    assert abs(l3[0] - float(lo[0])) < 1e-3
    named = dict(m1.named_parameters())
    a = torch.cat([named[k].grad.flatten() for k in go if k.startswith('wm.')]).double().cpu()
    b = torch.cat([go[k].flatten() for k in go if k.startswith('wm.')]).double()
    cos = float((a @ b) / (a.norm() * b.norm()))
    print('bf16 vs fp32 oracle: loss_model', l1[0], float(lo[0]), 'wm grad cosine', cos)
    assert cos > 0.999


def test_pack_metrics(hip):
    from pydreamer_amd.models import pack_metrics
    a = dict(x=torch.tensor(1.5, device=DEV), y=torch.tensor(-2.0, device=DEV))
    b = dict(z=torch.tensor([3.0], device=DEV))
    names, packed = pack_metrics(a, b)
    assert names == ['x', 'y', 'z'] and packed.tolist() == [1.5, -2.0, 3.0] and packed.is_cuda


def test_metric_buffer_and_lazy_tensors(hip):
    """(1) every loss / metric scalar of a step, and the four gradient norms, sit in ONE device buffer
    (Dreamer.packed_metrics) - parity of that buffer against the oracle's metrics at the loss tolerances; (2) `image_rec` is
    not materialised unless somebody reads it, and when read it equals the oracle's reconstruction."""
    from pydreamer_amd.models import METRIC_SLOTS
    oconf = O.tiny_conf()
    params = O.make_params(oconf)
    model = _build(oconf, params)
    conf = _hip_conf(oconf)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    obs = O.preprocess(O.synthetic_batch(oconf), oconf)
    noise = O.make_noise(oconf)
    losses, _, metrics, tensors, _ = model.training_step(_to_dev(obs), model.init_state(oconf.batch_size), noise=_to_dev(noise))
    assert not tensors.is_materialised('image_rec')
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    gm = model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
    names, buf, idx = model.packed_metrics()
    host = buf.tolist()                                                # ONE device->host copy for everything
    vals = dict(zip(names, (host[i] for i in idx)))
    ora = O.OracleDreamer(oconf, params)
    ora.init_optimizers()
    lo, _, mo, to, _ = ora.training_step(obs, ora.init_state(oconf.batch_size), noise)
    gmo, _ = ora.backward_clip_step(lo)
    for k, v in mo.items():
        assert k in vals, k
        assert abs(vals[k] - float(v)) <= 2e-5 * abs(float(v)) + 2e-6, (k, vals[k], float(v))
    for k, v in gmo.items():
        assert abs(vals[k] - float(v)) <= 1e-3 * abs(float(v)) + 1e-6, (k, vals[k], float(v))
    for k, v in {**metrics, **gm}.items():                            # the dict views alias the same buffer
        assert float(v) == vals[k], k
    assert set(METRIC_SLOTS) == set(names)
    rec = tensors['image_rec']
    assert tensors.is_materialised('image_rec') and rec.shape == to['image_rec'].shape
    _close(rec, to['image_rec'], 1e-4, 2e-5, 'lazy image_rec')
    assert dict(tensors)['image_rec'] is rec                            # plain-dict conversion resolves, never leaks a thunk


def test_optimizer_detects_rehomed_parameters(hip):
    """moving / casting the model after init_optimizers() must fail loudly instead of training a dead copy."""
    from pydreamer_amd.optim import FusedAdamW
    w = torch.nn.Parameter(torch.randn(10, 7, device=DEV))
    opt = FusedAdamW([w], lr=1e-3)
    opt.zero_grad()
    w.grad.add_(1.0)
    opt.step()                                    # fine
    w.data = w.data.clone()                       # what model.to(...) / .float() / load_state_dict(assign=True) do
    with pytest.raises(Exception) as e:
        opt.step()
    assert 'flat buffer' in str(e.value)


def test_optimizer_state_dict_is_torch_adamw_format(hip):
    """Checkpoint interop (tools.py:164-197 saves `optimizer_{i}_state_dict` = torch.optim.AdamW.state_dict()): FusedAdamW
    emits and accepts exactly that per-parameter layout.  (a) a torch AdamW loads the dict written by FusedAdamW and takes the
    same next step; (b) FusedAdamW loads the dict written by torch AdamW and takes the same next step; (c) round trip."""
    from pydreamer_amd.optim import FusedAdamW
    torch.manual_seed(5)
    shapes = [(7, 5), (13,), (3, 4, 2), (1,)]
    gen = lambda: [torch.randn(*s_) for s_ in shapes]
    init, grads = gen(), [gen() for _ in range(4)]
    pf = [torch.nn.Parameter(x.clone().to(DEV)) for x in init]
    pt = [torch.nn.Parameter(x.clone()) for x in init]
    fused = FusedAdamW(pf, lr=3e-3, eps=1e-5)
    ref = torch.optim.AdamW(pt, lr=3e-3, eps=1e-5)

    def step(opt, params, gs, dev):
        opt.zero_grad()
        for p_, g_ in zip(params, gs):
            if p_.grad is None:
                p_.grad = g_.to(dev).clone()
            else:
                p_.grad.copy_(g_.to(dev))
        opt.step()
    for i in range(2):
        step(fused, pf, grads[i], DEV)
        step(ref, pt, grads[i], 'cpu')
    sd = fused.state_dict()
    assert set(sd) == {'state', 'param_groups'} and sd['param_groups'][0]['params'] == [0, 1, 2, 3]
    assert set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'} and float(sd['state'][0]['step']) == 2.0
    # (a) torch loads ours
    pt2 = [torch.nn.Parameter(p_.detach().cpu().clone()) for p_ in pf]
    ref2 = torch.optim.AdamW(pt2, lr=1.0)
    ref2.load_state_dict({'state': {k: {kk: vv.cpu() if torch.is_tensor(vv) else vv for kk, vv in v.items()}
                                    for k, v in sd['state'].items()}, 'param_groups': sd['param_groups']})
    assert ref2.param_groups[0]['lr'] == 3e-3
    step(ref2, pt2, grads[2], 'cpu')
    step(ref, pt, grads[2], 'cpu')
    for a, b in zip(pt2, pt):
        assert float((a - b).abs().max()) < 2e-6
    # (b) ours loads torch's
    pf2 = [torch.nn.Parameter(p_.detach().clone().to(DEV)) for p_ in pt]
    fused2 = FusedAdamW(pf2, lr=1.0)
    fused2.load_state_dict(ref.state_dict())
    assert fused2.step_count == 3 and fused2.param_groups[0]['lr'] == 3e-3
    step(fused2, pf2, grads[3], DEV)
    step(ref, pt, grads[3], 'cpu')
    for a, b in zip(pf2, pt):
        assert float((a.cpu() - b).abs().max()) < 2e-6
    # (c) round trip through our own format is exact
    fused3 = FusedAdamW([torch.nn.Parameter(p_.detach().clone()) for p_ in pf2], lr=1.0)
    fused3.load_state_dict(fused2.state_dict())
    assert torch.equal(fused3.exp_avg, fused2.exp_avg) and torch.equal(fused3.exp_avg_sq, fused2.exp_avg_sq)
    assert fused3.step_count == fused2.step_count


def test_inference_matches_reference_golden(hip):
    """Dreamer.inference (dreamer.py:92-111; what generator.py:317-331 calls in the acting process) against
    tests/golden/tiny_inference.npz written by the real reference: action probabilities 2e-5, new state, policy_value.
    Together with tests/test_host_cpu.py::test_reference_loads_build_state_dict (build container only) this is the
    checkpoint path between a learner on this build and actors on the reference."""
    g = np.load(os.path.join(GOLD, 'tiny_inference.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    model = _build(oconf, O.make_params(oconf, seed=0))
    assert list(model.state_dict().keys()) == [str(k) for k in g['state_dict_keys']]
    u8 = torch.from_numpy(g['in_image_u8'])
    obs = dict(image=(u8.float() / 255.0 - 0.5).permute(0, 1, 4, 2, 3).contiguous().to(DEV), action=torch.from_numpy(g['in_action']).to(DEV),
               reset=torch.from_numpy(g['in_reset']).to(DEV))
    state = (torch.from_numpy(g['in_h']).to(DEV), torch.from_numpy(g['in_z']).to(DEV))
    with torch.no_grad():
        dist, (h1, z1), metrics = model.inference(obs, state, noise=dict(u_post=torch.from_numpy(g['in_u']).to(DEV)))
    _close(dist.probs, torch.from_numpy(g['action_probs']), 1e-4, 2e-6, 'action probabilities')
    _close(h1, torch.from_numpy(g['out_h']), 0, 2e-6, 'out_state h')
    assert torch.equal(z1.cpu(), torch.from_numpy(g['out_z']))
    assert abs(float(metrics['policy_value']) - float(g['policy_value'])) < 2e-6


@pytest.mark.parametrize('fixture', ['tiny_amp', 'atari_literal_amp', 'dmc_native_amp'])
def test_amp_against_reference_autocast_golden(hip, fixture):
    """tests/golden/tiny_amp.npz, atari_literal_amp.npz (BASELINE configs[2] at FULL size: B=50, T=50, H=15, deter 600) and
    dmc_native_amp.npz (BASELINE configs[4] as named: defaults+dmc, deter_dim 2048, tanh_normal actor on 6 continuous action
    dims, actor_grad=reinforce, B=50, T=50, H=15):
    the real reference's forward under torch.autocast('cpu', bfloat16) (its amp switch, train.py:166) and in fp32 on the
    same batch.  The build's mixed-precision mode rounds GEMM operands only (autocast also rounds layer outputs), so this
    is a loose pin - the bf16 tolerance this mode actually holds: with the posterior indices teacher-forced to the
    reference's, loss_model within 1e-3 relative of the reference's bf16 value AND of its fp32 value; the component
    metrics within 2e-2."""
    g = np.load(os.path.join(GOLD, fixture + '.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    obs = _to_dev(O.preprocess(O.synthetic_batch(oconf, seed=1234, first=True), oconf))
    noise = _to_dev(O.make_noise(oconf, seed=777))
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    try:
        section = 'dmc' if fixture.startswith('dmc') else 'atari'
        conf = config.load_config('defaults', section, **{**{k: getattr(oconf, k) for k in vars(oconf)}, 'amp': True})
        if section == 'dmc':
            assert conf.deter_dim == 2048 and conf.actor_dist == 'tanh_normal' and conf.action_dim == 6
        model = Dreamer(conf)
        model.load_state_dict(O.make_params(oconf, seed=0), strict=True)
        model = model.to(DEV)
        fidx = torch.from_numpy(g['bf16_idx_post'].astype(np.int64)).to(DEV)
        with torch.no_grad():
            losses, _, metrics, _, _ = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise,
                                                           forced_idx=fidx)
    finally:
        pass        # precision is a per-call argument: nothing to restore
    ref_bf16, ref_fp32 = float(g['bf16_losses'][0]), float(g['fp32_losses'][0])
    print('loss_model: build amp', float(losses[0]), 'reference autocast', ref_bf16, 'reference fp32', ref_fp32)
    assert abs(float(losses[0]) - ref_bf16) < 1e-3 * ref_bf16
    assert abs(float(losses[0]) - ref_fp32) < 1e-3 * ref_fp32
    for k in ('loss_image', 'loss_reward', 'loss_terminal', 'entropy_post'):
        assert _rel(metrics[k], float(g['bf16_metric_' + k])) < 2e-2, k


@pytest.mark.parametrize('fixture', ['atari_literal_amp', 'dmc_native_amp'])
def test_amp_gradients_against_reference_autocast_golden(hip, fixture):
    """The GRADIENT side of the mixed-precision pin (BASELINE configs[2] / [4] at full size): tests/golden/<fixture>_grads.npz holds
    the real reference's per-parameter gradient norms of the same step run under torch.autocast('cpu', bfloat16) WITH its four
    backward passes (oracle/gen_golden.py run_amp_grads; the losses in it equal the forward fixture's, same inputs and
    uniforms).  The build's amp mode (bf16 MFMA operands, fp32 accumulation and storage) against it, posterior indices
    teacher-forced to the reference's: loss_model within 1e-3 relative, every WORLD-MODEL parameter's gradient norm within the
    bf16-class bar below (autocast also rounds every layer OUTPUT to bf16, the build does not; the actor / critic gradients
    follow sampled imagination actions, which bf16 logits legitimately flip, so they are pinned by the fp32 fixtures only)."""
    path = os.path.join(GOLD, fixture + '_grads.npz')
    if not os.path.exists(path):
        pytest.skip(f'{path} not generated (oracle/gen_golden.py {fixture.split("_")[0]}_amp_grads: minutes of CPU)')
    g = np.load(path)
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    obs = _to_dev(O.preprocess(O.synthetic_batch(oconf, seed=1234, first=True), oconf))
    noise = _to_dev(O.make_noise(oconf, seed=777))
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    section = 'dmc' if fixture.startswith('dmc') else 'atari'
    conf = config.load_config('defaults', section, **{**{k: getattr(oconf, k) for k in vars(oconf)}, 'amp': True})
    model = Dreamer(conf)
    model.load_state_dict(O.make_params(oconf, seed=0), strict=True)
    model = model.to(DEV)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    fidx = torch.from_numpy(g['bf16_idx_post'].astype(np.int64)).to(DEV)
    losses, _, metrics, _, _ = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise, forced_idx=fidx)
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    torch.cuda.synchronize()
    assert abs(float(losses[0]) - float(g['bf16_losses'][0])) < 1e-3 * float(g['bf16_losses'][0])
    named = dict(model.named_parameters())
    errs = {str(n): abs(float(named[str(n)].grad.double().norm()) - r) / max(r, 1e-7)
            for n, r in zip(g['bf16_grad_names'], g['bf16_grad_norms']) if str(n).startswith('wm.')}
    worst = max(errs, key=errs.get)
    print(fixture, 'worst world-model grad-norm rel err vs the reference autocast backward:', worst, errs[worst],
          'median', float(np.median(list(errs.values()))))
    assert errs[worst] < 5e-2, (worst, errs[worst])
    # ... and the MEDIAN over the world-model parameters (the worst-case bar is 2x the measurement on two tiny
    # bias vectors and 50x on everything else): measured 4e-4 (atari_literal_amp) / 9e-4 (dmc_native_amp)
    med = float(np.median(list(errs.values())))
    assert med < 2e-3, (fixture, med)
    # 90 % of the parameters within 1e-2 (the tail is the bias vectors of the last head layers, whose gradients are sums of
    # 2 500 bf16-rounded terms that nearly cancel)
    p90 = float(np.quantile(list(errs.values()), 0.9))
    print(fixture, 'p90', p90)
    assert p90 < 1e-2, (fixture, p90)
